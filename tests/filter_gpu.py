"""What the GPU tests of the three byte-frame filters share (tests/test_area_gpu.py, tests/test_crop_area_gpu.py, tests/test_dof_gpu.py,
tests/test_filter_sweeps_gpu.py): one raw call of kbe_area_reduce_u8, kbe_crop_area_u8 and kbe_dof_u8 each, on buffers that all come from
guarded.Guard -- the source rows padded and the source moved off its allocation's start, the outputs in an allocation of their own per frame,
every byte the poison, the bands checked after the call."""
import ctypes

import numpy as np
import torch

from guarded import SENTINEL, Guard

POISONS = (0x00, 0xFF)


def stream():
    from ken_burns_effect_amd import _native
    return _native._stream()


current_stream = stream            # (the raw calls below take a `stream` of their own: the kbe_stream_t of the call, default torch's current stream)


def _padded_rows(frames, pad, gap=0):
    """uint8 [n,H,W,3] -> uint8 [n, H * (3 W + pad) + gap]: the rows `pad` bytes apart beyond their pixels, the frames `gap` bytes, 0x5A between."""
    n, H, W, _ = frames.shape
    rows = np.full((n, H * (3 * W + pad) + gap), 0x5A, np.uint8)
    rows[:, :H * (3 * W + pad)].reshape(n, H, 3 * W + pad)[:, :, :3 * W] = frames.reshape(n, H, 3 * W)
    return rows


def _placed(guard, rows, src_shift, outs_of, shift, aligned):
    """The source bytes `src_shift` bytes off a guarded allocation's start and one guarded output of outs_of bytes per frame, `shift` off its own.
    aligned: assert what the alignment classes of a sweep are computed from -- an allocation starts on a multiple of 512."""
    src = guard.empty((rows.size,), torch.uint8, 'cuda', shift=src_shift)
    src.copy_(torch.from_numpy(rows.reshape(-1)))
    outs = [guard.empty((outs_of,), torch.uint8, 'cuda', shift=shift) for _ in range(len(rows))]
    if aligned:
        assert src.data_ptr() % 512 == src_shift and all(o.data_ptr() % 512 == shift for o in outs)
    return src, outs


def run_area(A, frames, w, h, pad=0, out_pad=0, shift=0, src_shift=0, change=None, poison=SENTINEL, aligned=False, stream=None):
    """kbe_area_reduce_u8 on uint8 frames [n,H,W,3]: the source `src_shift` bytes off its allocation's start and its rows `pad` bytes apart
    beyond their pixels, the output's rows `out_pad`, the output `shift` bytes off its allocation's start, in a guarded allocation of its own
    per frame, every byte the poison (by default the bands' own byte).  change(args): the last word on the argument list -- a dict by the
    header's names.  -> (rc, [n, h, out_stride] bytes: the outputs as they lie)."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    rows = _padded_rows(frames, pad)
    guard = Guard(poison)
    out_stride = 3 * w + out_pad
    src, outs = _placed(guard, rows, src_shift, h * out_stride, shift, aligned)
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[src.data_ptr() + i * H * (3 * W + pad) for i in range(n)]), n_frames=n, W=W, H=H, stride_bytes=3 * W + pad,
                out_u8=(ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), w=w, h=h, out_stride_bytes=out_stride, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = A._raw('kbe_area_reduce_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly h * out_stride bytes between untouched bands
    return rc, np.stack([o.cpu().numpy().reshape(h, out_stride) for o in outs])


def run_crop_area(CA, frames, crop, size, pad=0, out_pad=0, shift=0, src_shift=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_crop_area_u8 on uint8 frames [n,H,W,3]: the source `src_shift` bytes off its allocation's start and its rows `pad` bytes apart beyond
    their pixels, the output's rows `out_pad`, the output `shift` bytes off its allocation's start, in a guarded allocation of its own per
    frame, every byte the poison.  change(args): the last word on the argument list -- a dict by the header's names.
    -> (rc, [n, h, out_stride] bytes: the outputs as they lie)."""
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
    rc = CA._raw('kbe_crop_area_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly h * out_stride bytes between untouched bands
    return rc, np.stack([o.cpu().numpy().reshape(h, out_stride) for o in outs])


def run_dof(DOF, frames, depths, focus, A, R, pad=0, z_pad=0, out_pad=0, shift=0, src_shift=0, gap=0, change=None, poison=0xFF, aligned=False, stream=None):
    """kbe_dof_u8 on uint8 frames [n,H,W,3] and float32 depths [n,H,W]: the source `src_shift` bytes off its allocation's start, its rows `pad`
    bytes apart beyond their pixels and its frames `gap` bytes apart, the depth rows `z_pad` floats apart, the output's rows `out_pad` bytes,
    the output `shift` bytes off its allocation's start, in a guarded allocation of its own per frame, every byte the poison.
    change(args): the last word on the argument list -- a dict by the header's names.  -> (rc, [n, H, out_stride] bytes: the outputs as they lie)."""
    frames, depths = np.asarray(frames), np.asarray(depths, np.float32)
    n, H, W, _ = frames.shape
    rows = _padded_rows(frames, pad, gap)
    planes = np.full((n, H, W + z_pad), -7.0, np.float32)
    planes[:, :, :W] = depths
    guard = Guard(poison)
    out_stride = 3 * W + out_pad
    src, outs = _placed(guard, rows, src_shift, H * out_stride, shift, aligned)
    z = guard.empty((planes.size,), torch.float32, 'cuda')
    z.copy_(torch.from_numpy(planes.reshape(-1)))
    args = dict(frames_u8=(ctypes.c_void_p * n)(*[src.data_ptr() + i * rows.shape[1] for i in range(n)]),
                depth_f32=(ctypes.c_void_p * n)(*[z.data_ptr() + 4 * i * H * (W + z_pad) for i in range(n)]), n_frames=n, W=W, H=H, stride_bytes=3 * W + pad,
                depth_stride_floats=W + z_pad, focus=(ctypes.c_double * n)(*[float(f) for f in focus]), aperture=float(A), max_radius=R,
                out_u8=(ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), out_stride_bytes=out_stride, stream=current_stream() if stream is None else stream)
    if change:
        change(args)
    rc = DOF._raw('kbe_dof_u8', *args.values())
    torch.cuda.synchronize()
    guard.check()                                                       # exactly H * out_stride bytes between untouched bands
    assert np.array_equal(src.cpu().numpy(), rows.reshape(-1)) and np.array_equal(z.cpu().numpy().view(np.uint8), planes.reshape(-1).view(np.uint8))          # the inputs are only read (bit for bit: NaNs among them)
    return rc, np.stack([o.cpu().numpy().reshape(H, out_stride) for o in outs])
