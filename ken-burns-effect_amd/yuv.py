"""Video planes: every frame of a clip as planar Y'CbCr 4:2:0 -- BT.601 at limited range, 1.5 bytes a pixel instead of 3 --, converted on the
GPU from frames that lie in HBM (include/kbe_yuv.h: kbe_yuv420_u8; the arithmetic is defined in csrc/kbe_yuv_block.h), and written as the one
uncompressed format that video encoders and players read: a YUV4MPEG2 file (write_y4m; Pipeline(y4m=True), kbe.py --y4m).  Half the bytes of
the RGB frames cross the link.

A frame's payload is its Y plane (H rows of W), its Cb plane and its Cr plane (ch rows of cw each; chroma_size), frame_bytes in all: the bytes
that follow "FRAME\\n" in a C420jpeg stream, the chroma sited at the centre of its 2 x 2 pixels.

This is the only module that names the entries of kbe_yuv.h: they are exported by libkbe_hip.so beside those of the other headers and typed
from their own header on the package's one handle of that library, the way the other frame filters' modules type their own.  No fallback:
without the HIP library every call here raises.
"""
import ctypes
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_yuv.h')
ABI_VERSION = 1
KBE_YUV_BGR = 1
FRAMES_PER_LAUNCH = 12             # KBE_YUV_FRAMES_PER_LAUNCH: the entry cuts a call's frames into launches of this many
MAX_SIDE = 65535
HEADER = _cabi.Header(HEADER_PATH, 'KBE_YUV_API', 'include/kbe_yuv.h', abi=('kbe_yuv_abi_version', ABI_VERSION, 'yuv '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_yuv.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its entries of include/kbe_yuv.h typed from that header the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_yuv.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def chroma_size(W, H):
    """(cw, ch): the cells of a chroma plane, one for every 2 x 2 pixels and for what is left of them at an odd width or height."""
    return (int(W) + 1) // 2, (int(H) + 1) // 2


def frame_bytes(W, H):
    """The bytes of one frame's payload, W H + 2 cw ch, as the library counts them; 0 where W or H is outside 1..65535."""
    return int(_raw('kbe_yuv420_bytes', int(W), int(H)))


def convert(frames_in_hbm, bgr=False):
    """uint8 [n,H,W,3] frames in HBM -> a new uint8 [n, frame_bytes(W, H)] tensor on the same device, every row a frame's payload.  bgr: a
    pixel's bytes are B, G, R.  Asynchronous on the current stream."""
    import torch
    f = frames_in_hbm
    if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 4 and f.size(3) == 3 and f.size(0) >= 1 and f.is_contiguous()):
        raise _native.KbeError('yuv.convert takes a contiguous uint8 [n,H,W,3] tensor on the GPU (got %s)' % (
            '%s %s on %s' % (tuple(f.shape), f.dtype, f.device) if torch.is_tensor(f) else type(f).__name__))
    n, H, W, _, sources = _native.frame_pointers(f, 'yuv.convert')
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise _native.KbeError('yuv.convert: frames of %d x %d: 1..%d either way' % (W, H, MAX_SIDE))
    size = frame_bytes(W, H)
    out = torch.empty((n, size), dtype=torch.uint8, device=f.device)
    targets = (ctypes.c_void_p * n)(*[out.data_ptr() + i * size for i in range(n)])
    _call('kbe_yuv420_u8', sources, n, W, H, 3 * W, targets, KBE_YUV_BGR if bgr else 0, _native._stream())
    return out


def planes(payload, W, H):
    """(Y [H,W], Cb [ch,cw], Cr [ch,cw]) as views of one frame's payload, a NumPy array or a tensor of frame_bytes(W, H) bytes."""
    cw, ch = chroma_size(W, H)
    if tuple(payload.shape) != (W * H + 2 * cw * ch,):
        raise ValueError('yuv.planes: a payload of %s for frames of %d x %d: %d bytes' % (tuple(payload.shape), W, H, W * H + 2 * cw * ch))
    return payload[:W * H].reshape(H, W), payload[W * H:W * H + cw * ch].reshape(ch, cw), payload[W * H + cw * ch:].reshape(ch, cw)


def y4m_header(W, H, fps=25):
    """The stream header of a YUV4MPEG2 file of W x H frames at fps frames a second, progressive, square pixels, 4:2:0 with the chroma at the
    cells' centres, limited range.  A frame rate that is no whole number is written as a fraction over 1000."""
    fps = float(fps)
    if not 0.0 < fps < float('inf'):
        raise ValueError('yuv.y4m_header: fps = %r: frames a second, above 0' % (fps,))
    num, den = (int(fps), 1) if fps == int(fps) else (int(round(fps * 1000)), 1000)
    return b'YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n' % (int(W), int(H), num, den)


def write_y4m(path, frames_in_hbm, fps=25, bgr=False, back=True):
    """The frames as a YUV4MPEG2 file: converted where they lie in HBM, the payloads fetched once into pinned memory -- half the frames' bytes
    --, then the header and "FRAME\\n" + payload for every frame.  back: the clip plays forth and back as the video does (frames +
    frames[-2::-1]), the way back being the same payload bytes again.  The file is opened 'wb': a FIFO at `path` works.
    -> the number of frames in the file"""
    import torch
    payloads = convert(frames_in_hbm, bgr=bgr)
    host = torch.empty(payloads.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(payloads, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    rows = host.numpy()
    n, H, W = frames_in_hbm.shape[:3]
    order = list(range(n)) + (list(range(n - 2, -1, -1)) if back else [])
    with open(path, 'wb') as f:
        f.write(y4m_header(W, H, fps))
        for i in order:
            f.write(b'FRAME\n')
            f.write(memoryview(rows[i]))
    return len(order)
