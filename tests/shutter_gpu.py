"""What the GPU tests of the shutter mean share (tests/test_shutter_gpu.py): one raw call of kbe_shutter_mean_u8 on buffers that all come from
guarded.Guard -- the source rows padded and the source moved off its allocation's start, the outputs in an allocation of their own per frame,
every byte the poison, the bands checked after the call -- the way tests/filter_gpu.py calls the other byte-frame filters."""
import ctypes

import numpy as np
import torch

from filter_gpu import _padded_rows, current_stream
from guarded import Guard

POISONS = (0x00, 0xFF)
SPAN = 1024          # csrc/kbe_shutter.hip, kSpan: the bytes of a row, counted from the row's address rounded down to 16, that one workgroup takes


def run_shutter(SH, frames, S, table=None, pad=0, out_pad=0, shift=0, src_shift=0, gap=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_shutter_mean_u8 on uint8 source frames [m,H,W,3]: the sources `src_shift` bytes off their allocation's start, their rows `pad` bytes
    apart beyond their pixels and the frames `gap` bytes apart; table: the pointer table as indices into the frames, `S` for every output
    (default: all m frames in their order, m / S outputs: a table may name a frame more than once); the output's rows `out_pad` bytes apart,
    the output `shift` bytes off its allocation's start, in a guarded allocation of its own per frame, every byte the poison.
    change(args): the last word on the argument list -- a dict by the header's names.  -> (rc, [n_out, H, out_stride] bytes: the outputs as they lie)."""
    frames = np.asarray(frames)
    m, H, W, _ = frames.shape
    table = list(range(m)) if table is None else list(table)
    assert len(table) % S == 0 and len(table) >= S
    n_out = len(table) // S
    rows = _padded_rows(frames, pad, gap)
    guard = Guard(poison)
    out_stride = 3 * W + out_pad
    src = guard.empty((rows.size,), torch.uint8, 'cuda', shift=src_shift)
    src.copy_(torch.from_numpy(rows.reshape(-1)))
    outs = [guard.empty((H * out_stride,), torch.uint8, 'cuda', shift=shift) for _ in range(n_out)]
    if aligned:                            # what the alignment classes of a sweep are computed from: an allocation starts on a multiple of 512
        assert src.data_ptr() % 512 == src_shift and all(o.data_ptr() % 512 == shift for o in outs)
    args = dict(frames_u8=(ctypes.c_void_p * len(table))(*[src.data_ptr() + k * rows.shape[1] for k in table]), n_out=n_out, samples=S, W=W, H=H, stride_bytes=3 * W + pad,
                out_u8=(ctypes.c_void_p * n_out)(*[o.data_ptr() for o in outs]), out_stride_bytes=out_stride, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = SH._raw('kbe_shutter_mean_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly H * out_stride bytes between untouched bands
    assert np.array_equal(src.cpu().numpy(), rows.reshape(-1))          # the inputs are only read
    return rc, np.stack([o.cpu().numpy().reshape(H, out_stride) for o in outs])


def assert_mean(SH, samples, want=None, poisons=POISONS, **kw):
    """samples [n, S, H, W, 3] through the entry under both poisons: the twin's bytes (or `want`), the rows' padding unwritten."""
    import shutter_cases as sc
    samples = np.asarray(samples)
    n, S, H, W, _ = samples.shape
    want = sc.twin_mean(samples) if want is None else want
    for poison in poisons:
        rc, got = run_shutter(SH, samples.reshape(n * S, H, W, 3), S, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * W].reshape(n, H, W, 3), want), (W, H, S, poison, kw)
        assert (got[:, :, 3 * W:] == poison).all()                       # the rows' padding is not written
