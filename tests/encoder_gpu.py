"""What the GPU tests of the device-side encoders share (kbe_mjpeg_encode, kbe_png_encode: the encoders' common contract of include/kbe.h):
one descriptor per encoder, the harness that calls an entry through ctypes with sentinels around everything it may write, and smoke()'s
scene.  tests/test_encoders_gpu.py holds the contract against both; test_mjpeg_gpu.py and test_png_gpu.py what is one format's own."""
import collections
import ctypes
import functools

import numpy as np
import torch

import mjpeg_cases as mc
import png_cases as pc
from guarded import GUARD, SENTINEL, Guard           # (0xA5, 4096: the bands of the output buffer here are the harness's)

# fmt: kbe_<fmt>_encode, kbe_<fmt>_scratch_bytes, kbe_<fmt>_bound; cases: the CPU suite's module (CASES, case_frames, case_twin, BGR); own(name): the
# entry's arguments in front of the flags for that case; encode(K, frames, name, **kw): the tensor-level call; ladder: the case of the
# too-small-buffer test; refused: what else the entry refuses, as changes to a good call
Encoder = collections.namedtuple('Encoder', 'fmt cases own encode ladder refused')
MJPEG = Encoder('mjpeg', mc, lambda name: (mc.CASES[name][2],), lambda K, frames, name, **kw: K.mjpeg_encode(frames, mc.CASES[name][2], **kw), 'noise',
                [dict(own=(0, 0)), dict(own=(101, 0))])
PNG = Encoder('png', pc, lambda name: (), lambda K, frames, name, **kw: K.png_encode(frames, **kw), 'photo_like',
              [dict(W=65535, H=65535, stride=3 * 65535)])                   # a file of 2^31 bytes or more
ENCODERS = [MJPEG, PNG]


def kernels():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def on_device(frames):
    return frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()


def run(K, enc, frames, own, cap, W=None, stride=None, n=None, status_before=7, shift=0):
    """The entry on a uint8 device tensor [n,H,Wt,3] (W <= Wt: the rows' stride is Wt's) with a buffer of `cap` bytes (`shift` bytes off its
    allocation's start) followed by GUARD bytes, everything the call may write filled with sentinels first; own: the entry's integers up to
    the flags.  The scratch is exactly kbe_<fmt>_scratch_bytes, rounded up only to the 8 bytes its alignment check asks for, every byte of
    it 0xFF, between two guard bands of its own (tests/guarded.py) that the call must leave alone.  -> (rc, offsets, status, the buffer
    with its guard)."""
    count, H, Wt, _ = frames.shape
    W = Wt if W is None else W
    n = count if n is None else n
    step = H * Wt * 3
    pointers = (ctypes.c_void_p * max(n, 1))(*[frames.data_ptr() + i * step for i in range(n)])
    guard = Guard(poison=0xFF)
    scratch = guard.empty(((int(getattr(K.lib, 'kbe_%s_scratch_bytes' % enc.fmt)(W, H, max(n, 1))) + 7) // 8 * 8,), torch.uint8, 'cuda')
    out = torch.full((shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    offsets = torch.full((max(n, 1) + 1,), -1, dtype=torch.int64, device='cuda')
    status = torch.full((1,), status_before, dtype=torch.int32, device='cuda')
    rc = K.encode_raw(enc.fmt, pointers, n, W, H, 3 * Wt if stride is None else stride, own, scratch.data_ptr(), out.data_ptr() + shift, cap, offsets.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    guard.check()
    got = out.cpu().numpy()
    assert (got[:shift] == SENTINEL).all()
    return rc, offsets.cpu().tolist(), int(status.item()), got[shift:]


def sizes_of(want):
    return np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()


def assert_units(K, enc, frames, own, want, room=333, **kw):
    """The device's streams or files of `frames` are `want`, back to back; no byte in front of them or behind them is touched."""
    total = sum(len(s) for s in want)
    rc, offsets, status, buf = run(K, enc, on_device(frames), own, total + room, **kw)
    assert rc == 0 and status == 0
    assert offsets == sizes_of(want)
    assert buf[:total].tobytes() == b''.join(want)
    assert (buf[total:] == SENTINEL).all()


def assert_case(K, enc, name):
    """A case of the CPU suite, 1, 3 and 13 frames of different content (13: two launches, the offsets carry on), RGB and BGR."""
    dev = on_device(enc.cases.case_frames(name, 13))
    for flags in (0, enc.cases.BGR):
        want = enc.cases.case_twin(name, 13, flags)[0]
        for n in (1, 3, 13):
            assert_units(K, enc, dev[:n], enc.own(name) + (flags,), want[:n])


def tiled(h, w, seed):
    tile = mc.photo_like(256, 256, seed)
    return np.tile(tile, (-(-h // 256), -(-w // 256), 1))[:h, :w]


@functools.lru_cache(maxsize=None)
def rendered(K):
    """smoke()'s scene: two cameras, the frames left in HBM and delivered raw; rendered once per process."""
    from ken_burns_effect_amd import common, synthetic
    H, W = 96, 128
    image, disp = synthetic.make_rgbd(H, W, seed=0)
    depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
    oc = {'dblFocal': synthetic.FOCAL, 'dblBaseline': synthetic.BASELINE, 'intWidth': W, 'intHeight': H, 'objectDepthrange': synthetic.depthrange_of(depth),
          'tensorRawImage': image.cuda(), 'tensorRawDisparity': disp.cuda(), 'tensorRawDepth': depth.cuda()}
    oc['tensorRawPoints'] = K.depth_to_points(oc['tensorRawDepth'], synthetic.FOCAL).view(1, 3, -1)
    ofrom, oto = synthetic.default_windows(H, W)
    settings = {'dblSteps': [0.0, 1.0], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False, 'boolCrop': False}
    common._reset_inpa(oc)
    cams = common.frame_cameras(settings, oc)
    in_hbm = common.render_frames(cams, oc, None, keep_on_device=True)
    raw = common.render_frames(cams, oc, None)
    return in_hbm, raw
