"""What the GPU tests of the transitions share (tests/test_transition_gpu.py): one raw call of kbe_transition_u8 on buffers that all come from
guarded.Guard -- the `from` frames and the `to` frames in an allocation each, their rows padded and each moved off its allocation's start by
an offset of its own, the outputs in an allocation of their own per frame, every byte the poison, the bands checked after the call -- the way
tests/shutter_gpu.py calls the shutter mean."""
import ctypes

import numpy as np
import torch

from filter_gpu import _padded_rows, current_stream
from guarded import Guard

POISONS = (0x00, 0xFF)
SPAN = 1024          # csrc/kbe_transition.hip, kSpan: the bytes of a row, counted from the row's address rounded down to 16, that one workgroup takes


def run_transition(TR, frames_from, frames_to, kind, progress, softness=8, colour=0, pad=0, out_pad=0, shift=0, src_shift=0, to_shift=None, gap=0, same=False,
                   change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_transition_u8 on two sets of uint8 frames [n,H,W,3]: `from` `src_shift` bytes and `to` `to_shift` bytes (default: as `from`) off their
    allocations' starts, their rows `pad` bytes apart beyond their pixels and the frames `gap` bytes apart; same: the `to` table is the `from`
    table; the output's rows `out_pad` bytes apart, the output `shift` bytes off its allocation's start, in a guarded allocation of its own
    per frame, every byte the poison.  change(args): the last word on the argument list -- a dict by the header's names.
    -> (rc, [n, H, out_stride] bytes: the outputs as they lie)."""
    a, b = np.asarray(frames_from), np.asarray(frames_to)
    n, H, W, _ = a.shape
    assert b.shape == a.shape and len(progress) == n
    to_shift = src_shift if to_shift is None else to_shift
    guard = Guard(poison)
    out_stride = 3 * W + out_pad
    placed = []
    for frames, off in ((a, src_shift), (b, to_shift)):
        rows = _padded_rows(frames, pad, gap)
        t = guard.empty((rows.size,), torch.uint8, 'cuda', shift=off)
        t.copy_(torch.from_numpy(rows.reshape(-1)))
        placed.append((t, rows))
    outs = [guard.empty((H * out_stride,), torch.uint8, 'cuda', shift=shift) for _ in range(n)]
    if aligned:                            # what the alignment classes of a sweep are computed from: an allocation starts on a multiple of 512
        assert placed[0][0].data_ptr() % 512 == src_shift and placed[1][0].data_ptr() % 512 == to_shift and all(o.data_ptr() % 512 == shift for o in outs)
    tables = [(ctypes.c_void_p * n)(*[t.data_ptr() + k * rows.shape[1] for k in range(n)]) for t, rows in placed]
    args = dict(from_u8=tables[0], to_u8=tables[0] if same else tables[1], n=n, W=W, H=H, stride_bytes=3 * W + pad, kind=kind if isinstance(kind, int) else TR.KINDS[kind],
                progress=(ctypes.c_int32 * n)(*progress), softness=softness, colour=colour, out_u8=(ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]),
                out_stride_bytes=out_stride, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = TR._raw('kbe_transition_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly H * out_stride bytes between untouched bands
    for t, rows in placed:
        assert np.array_equal(t.cpu().numpy(), rows.reshape(-1))        # the inputs are only read
    return rc, np.stack([o.cpu().numpy().reshape(H, out_stride) for o in outs])


def assert_blend(TR, frames_from, frames_to, kind, progress, want=None, softness=8, colour=0, poisons=POISONS, **kw):
    """Two sets of frames through the entry under both poisons: the twin's bytes (or `want`), the rows' padding unwritten."""
    import transition_cases as tc
    a, b = np.asarray(frames_from), np.asarray(frames_to)
    n, H, W, _ = a.shape
    want = tc.twin_blend(a, a if kw.get('same') else b, kind, progress, softness, colour) if want is None else want
    for poison in poisons:
        rc, got = run_transition(TR, a, b, kind, progress, softness, colour, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * W].reshape(n, H, W, 3), want), (W, H, kind, progress, softness, poison, kw)
        assert (got[:, :, 3 * W:] == poison).all()                       # the rows' padding is not written
