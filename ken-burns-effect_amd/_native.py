"""ctypes binding of ``csrc/libkbe_hip.so`` (C ABI: ``include/kbe.h``).

This is the only compute back end of the package.  There is deliberately no CPU or
PyTorch fallback: :func:`load` raises if the library is missing, and every wrapper
refuses tensors that are not contiguous fp32 CUDA(=HIP) tensors.

The wrappers take torch tensors only to obtain ``data_ptr()`` and the current HIP
stream -- the same contract the reference had with CuPy
(``/root/reference/utils/common.py:516-521``), minus the per-shape JIT.

The types of every entry come from the header (:func:`prototypes`, ``_cabi``): :func:`load` sets them, the wrappers pass plain
Python values through :meth:`HipKernels._call`, and a call that does not fit the header is refused before it is made.
"""
import ctypes
import os

import torch

from . import _cabi, video_shape
from ._cabi import KbeError
# (the flag bits under the header's names, and the rules and thresholds of a video call's shape that lived here before video_shape.py did)
from .video_shape import (DEFAULT_FILL_GROUP, DEFAULT_HOST_LANES, FUSED_DENSE, FUSED_HOST_GROUP, KBE_STAGE_FUSED_LEAN, KBE_STAGE_FUSED_ROOMY,  # noqa: F401
                          KBE_STAGE_PROJECT, KBE_VIDEO_FILL_DIST, KBE_VIDEO_FILL_GROUP, KBE_VIDEO_GROUP, KBE_VIDEO_FREE_TRANSFERS,
                          KBE_VIDEO_EVEN_GROUPS, KBE_VIDEO_NO_AHEAD, KBE_VIDEO_FAST_RAMP, KBE_VIDEO_FUSED_LEAN, KBE_VIDEO_FUSED_ROOMY, KBE_VIDEO_SDMA,
                          KBE_VIDEO_INJECT_FAULT, KBE_VIDEO_INJECT_TIMEOUT, LINK_BYTES_PER_US, Switches, lanes_for_delivery, transfer_group)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('KBE_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libkbe_hip.so')      # (KBE_LIB_PATH: a variant build of the same ABI -- measurements)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'kbe.h')     # the contract: every entry's types are read from it (prototypes)

ABI_VERSION = 13
MAX_LANES = 8          # KBE_MAX_LANES
KBE_MJPEG_BGR = 1      # kbe_mjpeg_encode flags
KBE_PNG_BGR = 1        # kbe_png_encode flags
DEFAULT_LANES = 4      # streams the frame loop spreads consecutive frames over (env KBE_LANES)
FUSED_MAX_DENSITY = 20.0         # clouds up to this many points per pixel take the fused scatter by default (KBE_FUSED=auto).  Round 5: a tile's candidate list holds 2048
                                 # sub-blocks (512 before: the densest tiles' lists overflowed from 5 points per pixel on and those tiles scanned the cloud) and a record
                                 # that finds no room in LDS waits as its 4-byte point index (16-byte records before; four times the capacity) -- the route now grows
                                 # linearly to 20 points per pixel: 141 / 284 / 395 / 535 / 657 us per 1024^2 frame at 4 / 9 / 12 / 16 / 20 per pixel, 11.6 ms at 24
                                 # (profiles/r05_density_sweep.txt; the bucket route: 153 / 14 083 us at 4 / 9, the atomic kernels 2.1 / 5.2 / 20.5 ms at 4 / 9 / 24).
                                 # (4.5 in round 4, 1.5 before.)
FUSED_MAX_POINTS = 1 << 28       # the packed cloud's route addresses points by 32-bit byte offsets (KBE_FUSED_MAX_POINTS, kbe_tiles.h): larger clouds take the bucket route
PROBE_MIN_FRAMES = 128 # delivered videos from this length on have their lanes measured (HipKernels.delivery_lanes); shorter ones take the a-priori estimate


_LANE_STREAMS = {}


def lane_streams_of(device, n):
    """n streams for the lanes of the frame loop beside the caller's stream, one set per device for the life of the process: torch's own
    streams.  KBE_LANE_PRIORITY=1 (dev) makes them LOW-priority HIP streams: lane 0 -- the caller's stream -- renders a video's FIRST
    frame, which every byte of a short delivered video waits for, while lane 1 already renders the second group next to it; with the
    other lanes below it the first frame has the chip when both want it (tools/batches/gpu_r05_prio.sh, three processes each, k frames/s
    delivered: 20 frames 14.95 -> 15.02, 16 frames 14.28 -> 14.40; high-priority lanes 14.83 / 14.25; long videos and frames left in
    HBM: no difference).  NOT the default: with several processes on one GPU (tests/test_hip_parity.py: four ranks next to the test
    process) the low-priority queues are scheduled erratically -- passes of 3.5 to 24.6 ms where torch's streams give 7.0 +- 0.4."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device())
    have = _LANE_STREAMS.setdefault(key, [])
    while len(have) < n:
        stream = None
        if os.environ.get('KBE_LANE_PRIORITY', '0') == '1':
            try:
                hip = ctypes.CDLL('libamdhip64.so')
                least, greatest, handle = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p()
                with torch.cuda.device(key):
                    if hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) == 0 and least.value > 0 and \
                            hip.hipStreamCreateWithPriority(ctypes.byref(handle), ctypes.c_uint(1), least) == 0 and handle.value:      # 1 = hipStreamNonBlocking
                        stream = torch.cuda.ExternalStream(handle.value, device=torch.device('cuda', key))
            except (OSError, AttributeError, RuntimeError):
                stream = None
        have.append(stream if stream is not None else torch.cuda.Stream(device=torch.device('cuda', key)))
    return have[:n]


def forced_host_lanes():
    """KBE_HOST_LANES: the lanes of a delivered video, whatever the estimate or the probe would say (None: unset)."""
    env = os.environ.get('KBE_HOST_LANES')
    return int(env) if env else None


def host_lanes(lanes, n_points, W, H, frame_bytes):
    """video_shape.host_lanes, the a-priori estimate of a delivered video's lanes, under env KBE_HOST_LANES."""
    return video_shape.host_lanes(lanes, n_points, W, H, frame_bytes, forced_host_lanes())


_lib = None
HEADER = _cabi.Header(HEADER_PATH, 'KBE_API', 'include/kbe.h', abi=('kbe_abi_version', ABI_VERSION, ''))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe.h declares, in its order, read once


def __getattr__(name):
    if name == 'SYMBOLS':          # every symbol include/kbe.h declares (tests check the library exports exactly these)
        return tuple(prototypes())
    raise AttributeError('module %r has no attribute %r' % (__name__, name))


def load():
    """Loads the HIP library once and types every entry from the header; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KbeError('HIP extension not built: %s is missing. Run `python -c "import __graft_entry__ as g; g.build()"` '
                       '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
    _lib = HEADER.bind(ctypes.CDLL(LIB_PATH))
    return _lib


def _ptr(t, dtype=torch.float32):
    if t is None:
        return ctypes.c_void_p(0)
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise KbeError('kernel arguments must be contiguous %s tensors on the GPU (got %s %s on %s)'
                       % (dtype, 'contiguous' if t.is_contiguous() else 'strided', t.dtype, t.device))
    if t.device.index != torch.cuda.current_device():
        raise KbeError('tensor on %s but the current device is cuda:%d: wrap the call in torch.cuda.device(%d) '
                       '(launches go to the current device\'s stream)' % (t.device, torch.cuda.current_device(), t.device.index))
    return ctypes.c_void_p(t.data_ptr())


def _f32c(t):
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _shift(shift3):
    if shift3 is None:
        return None
    if torch.is_tensor(shift3):
        shift3 = shift3.detach().reshape(-1).tolist()     # 3 host floats (already fp32-representable)
    return (ctypes.c_float * 3)(*[float(v) for v in shift3])


def _stream():
    """The HIP stream launches go to: torch's current stream of the CURRENT device.  Every wrapper below checks that its
    tensors live on that device (`_ptr`), so a caller working on cuda:1 without torch.cuda.set_device(1) gets a KbeError
    instead of device-1 pointers launched on device 0's stream."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rect(fill_rect):
    return None if fill_rect is None else (ctypes.c_int * 4)(*[int(v) for v in fill_rect])


def _group_args(cameras, scratch, stride, out=None, fill_rect=None):
    """The argument arrays of a group of frames [(focal, shift3)], frame k on scratch set k: (focals, shifts, set pointers,
    frame pointers -- None without `out` --, fill rectangle)."""
    n = len(cameras)
    focals = (ctypes.c_double * n)(*[float(c[0]) for c in cameras])
    shifts = (ctypes.c_float * (3 * n))(*[float(v) for c in cameras for v in c[1]])
    sets = (ctypes.c_void_p * n)(*[scratch.data_ptr() + k * stride for k in range(n)])
    frames = None if out is None else (ctypes.c_void_p * n)(*[out[k].data_ptr() for k in range(n)])
    return focals, shifts, sets, frames, _rect(fill_rect)


def frame_pointers(frames, what):
    """A uint8 [n,H,W,3] tensor of frames on the GPU -> (n, H, W, the bytes of a frame, the array of the frames' addresses); `what`: the caller, for the refusal."""
    if not (torch.is_tensor(frames) and frames.dim() == 4 and frames.size(3) == 3 and frames.size(0) >= 1):
        raise KbeError('%s takes a uint8 [n,H,W,3] tensor on the GPU' % what)
    n, H, W, _ = frames.shape
    base, step = _ptr(frames, torch.uint8).value, H * W * 3
    return n, H, W, step, (ctypes.c_void_p * n)(*[base + i * step for i in range(n)])


def encode_units(what, name, frames, scratch_bytes, cap, first_guess, entry):
    """The whole of a tensor-level call of a unit encoder (the encoders' common contract, include/kbe.h; gif.py's entry keeps it too) -> the
    bytes of each frame's unit.  what, name: the caller and its entry, for messages; scratch_bytes: the entry's kbe_<fmt>_scratch_bytes;
    first_guess(n, the bytes of a frame): the buffer's size when `cap` is None; entry(frames, n, W, H, stride, scratch, out, cap, offsets,
    status, stream): the one call, which puts its own arguments where its header has them and raises unless KBE_OK.  One synchronisation
    for the offsets and the status word; units that do not fit are encoded once more into a buffer of the size the first run reported."""
    n, H, W, step, pointers = frame_pointers(frames, what)
    device = frames.device
    scratch = torch.empty((int(scratch_bytes(W, H, n)) + 7) // 8 + 1, dtype=torch.int64, device=device)
    meta = torch.empty(n + 2, dtype=torch.int64, device=device)          # offsets [n + 1], then the status word
    cap = int(cap) if cap is not None else first_guess(n, step)
    for attempt in (0, 1):
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
        entry(pointers, n, W, H, 3 * W, scratch.data_ptr(), out.data_ptr(), cap, meta.data_ptr(), meta.data_ptr() + 8 * (n + 1), _stream())
        host = meta.cpu()                                               # (the one synchronisation)
        offsets, overflow = host[:n + 1].tolist(), int(host[n + 1].item()) & 0xFFFFFFFF
        if not overflow:
            break
        if attempt == 1:
            raise KbeError('%s: %d bytes do not fit a buffer of %d' % (name, offsets[n], cap))
        cap = offsets[n]
    data = out[:offsets[n]].cpu().numpy()
    return [data[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]


_BUILD_BITS = {'lean': (KBE_STAGE_FUSED_LEAN, KBE_VIDEO_FUSED_LEAN), 'roomy': (KBE_STAGE_FUSED_ROOMY, KBE_VIDEO_FUSED_ROOMY)}


def fused_build_bits(video=False):
    """KBE_FUSED_CAP=lean|roomy (tests, measurements): the flag that forces one build of the fused route's tile launches
    (KBE_STAGE_FUSED_LEAN / _ROOMY, or the kbe_render_video form).  The environment is read HERE, per call; the library reads none."""
    bits = _BUILD_BITS.get(os.environ.get('KBE_FUSED_CAP'))
    return bits[1 if video else 0] if bits else 0


HANDOFF_DEFAULT = 'sdma'    # measured (profiles/r05_handoff_sdma.txt): 20 frames 14.1 k -> 14.5-14.8 k frames/s, 75 frames 16.4-16.5 -> 16.5-16.6 k, long videos equal (KBE_HANDOFF=sdma|blit)


def handoff_by_sdma():
    """Do a delivered video's frame groups leave through an SDMA engine (KBE_VIDEO_SDMA) or through hipMemcpyAsync (a blit kernel)?"""
    return os.environ.get('KBE_HANDOFF', HANDOFF_DEFAULT) == 'sdma'


def video_switches():
    """Every environment switch that shapes a video call (HipKernels.render_video), read once per call -- tests flip them between
    calls -- into a video_shape.Switches record; video_shape.call_shape decides by the record, nothing else of a call reads them.
    Defaults in brackets:
      KBE_FILL_DIST [auto] | 0 | 1         the table-driven hole fill (auto: a cloud without appended points seen by a camera that zooms out)
      KBE_FILL_GROUP [by route, frame size and destination]   frames per launch of a lane: 1..4 on the bucket route, 1..12 on the fused one
      KBE_HOST_LANES [estimated or measured]    lanes of a delivered video (forced_host_lanes: host_lanes and delivery_lanes take it too)
      KBE_DELIVERY_BATCH [0 = transfer_group]   frames per transfer: < 0 groups per lane, > 0 the staged ring
      KBE_RAMP [classic] | fast            transfer groups of 1, 2, 4, ... or 1, 3, 7, ... frames (KBE_VIDEO_FAST_RAMP)
      KBE_FREE_TRANSFERS [auto] | 0 | 1    the lanes do not take turns on the link (auto: with the table-driven fill)
      KBE_EVEN_GROUPS [0] | 1              (dev) transfer groups of one size, no ramp
      KBE_AHEAD [1] | 0                    0: every group of the fused route keeps its own placement launch (KBE_VIDEO_NO_AHEAD)
      KBE_FUSED_CAP lean | roomy           forces a build of the tile launches (fused_build_bits, which the one-frame and group entries use too)
      KBE_HANDOFF [sdma] | blit            how a delivered video's frame groups leave (handoff_by_sdma)
      KBE_INJECT_HANDOFF_FAULT, KBE_INJECT_HANDOFF_TIMEOUT = 1    test hooks of the SDMA hand-off
      KBE_SCRATCH_BUDGET_MB [half of the free device memory]      what the loop's scratch sets may take
    (KBE_SHARE_LISTS is near_depth's; KBE_LANES, KBE_FUSED and KBE_NO_RASTER_HINT are prepare_cloud's.)"""
    env = os.environ.get
    batch = env('KBE_DELIVERY_BATCH', '0')
    try:
        batch = int(batch)
    except ValueError:
        raise KbeError('KBE_DELIVERY_BATCH=%r is not an integer (frames per transfer: < 0 groups per lane, > 0 staged ring)' % batch)
    fill_dist, fill_group, free, budget = env('KBE_FILL_DIST', 'auto'), env('KBE_FILL_GROUP'), env('KBE_FREE_TRANSFERS', 'auto'), env('KBE_SCRATCH_BUDGET_MB')
    return Switches(fill_dist=None if fill_dist == 'auto' else fill_dist != '0', fill_group=int(fill_group) if fill_group else None,
                    host_lanes=forced_host_lanes(), delivery_batch=batch, fast_ramp=env('KBE_RAMP', 'classic') == 'fast',
                    free_transfers=None if free == 'auto' else free == '1', even_groups=env('KBE_EVEN_GROUPS') == '1', no_ahead=env('KBE_AHEAD') == '0',
                    build_bits=fused_build_bits(video=True), sdma=handoff_by_sdma(), inject_fault=env('KBE_INJECT_HANDOFF_FAULT') == '1',
                    inject_timeout=env('KBE_INJECT_HANDOFF_TIMEOUT') == '1', scratch_budget_mb=float(budget) if budget else None)


class HipKernels:
    """Tensor-level view of the C ABI.  One instance is shared by the package."""

    name = 'hip'

    def __init__(self):
        self.lib = load()
        self._tiled_scratch = {}      # (device, W, H) -> scratch of the tiled render_pointcloud

    def _check(self, rc, what):
        HEADER.check(self.lib, rc, what)

    def _raw(self, name, *args):
        """The entry `name` of include/kbe.h with plain Python values -> what it returns (_cabi.Header.raw: held to the header's types and
        argument count, looked up on self.lib at each call -- a tool may have put a shim there)."""
        return HEADER.raw(self.lib, name, *args)

    def _call(self, name, *args, what=None):
        """An entry that returns a status: KbeError with the library's text (under the label `what`, default the entry's name) unless KBE_OK."""
        self._check(self._raw(name, *args), what or name)

    def selftest_err(self, z, focal, baseline):
        z = _f32c(z).reshape(-1)
        fast, exact = torch.empty_like(z), torch.empty_like(z)
        self._call('kbe_selftest_err', _ptr(z), z.numel(), float(focal), float(baseline), _ptr(fast), _ptr(exact), _stream())
        return fast, exact

    def selftest_division(self, num, den):
        num, den = _f32c(num).reshape(-1), _f32c(den).reshape(-1)
        fast, ieee = torch.empty_like(num), torch.empty_like(num)
        self._call('kbe_selftest_division', _ptr(num), _ptr(den), num.numel(), _ptr(fast), _ptr(ieee), _stream())
        return fast, ieee

    # -- render_pointcloud and its stages ------------------------------------------------
    def zsplat(self, points, W, H, focal, baseline, shift3=None, want_winner=False):
        points = _f32c(points)
        B, _, N = points.shape
        zkeys = torch.empty(B, 1, H, W, dtype=torch.int32, device=points.device)
        self._call('kbe_zkeys_clear', _ptr(zkeys, torch.int32), zkeys.numel(), _stream())
        winner = torch.empty(B, N, dtype=torch.int32, device=points.device) if want_winner else None
        self._call('kbe_zsplat', _ptr(points), B, N, W, H, float(focal), float(baseline), _shift(shift3), _ptr(zkeys, torch.int32),
                   _ptr(winner, torch.int32), _stream())
        return zkeys, winner

    def zkeys_decode(self, zkeys):
        zee = torch.empty(zkeys.shape, dtype=torch.float32, device=zkeys.device)
        self._call('kbe_zkeys_decode', _ptr(zkeys, torch.int32), zkeys.numel(), _ptr(zee), _stream())
        return zee

    def degrid(self, zkeys=None, zee=None):
        src = zkeys if zkeys is not None else zee
        B, _, H, W = src.shape
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=src.device)
        self._call('kbe_degrid', _ptr(zkeys, torch.int32), _ptr(None if zee is None else _f32c(zee)), B, W, H, _ptr(out), _stream())
        return out

    def degrid_serial(self, zkeys=None, zee=None):
        """The serial (index-order, in-place) schedule of the same kernel: what the reference-run golden vectors hold.
        Proof-of-fidelity entry for the tests; the product path uses :meth:`degrid`'s out-of-place schedule."""
        src = zkeys if zkeys is not None else zee
        B, _, H, W = src.shape
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=src.device)
        self._call('kbe_degrid_serial', _ptr(zkeys, torch.int32), _ptr(None if zee is None else _f32c(zee)), B, W, H, _ptr(out), _stream())
        return out

    def accumulate(self, points, data, zee, focal, baseline, shift3=None):
        points, data = _f32c(points), _f32c(data)
        B, C, N = data.shape
        _, _, H, W = zee.shape
        acc = torch.zeros(B, C + 1, H, W, dtype=torch.float32, device=points.device)
        self._call('kbe_accumulate', _ptr(points), _ptr(data), B, N, C, _ptr(_f32c(zee)), W, H, float(focal), float(baseline), _shift(shift3),
                   _ptr(acc), _stream())
        return acc

    def normalize(self, acc):
        B, C1, H, W = acc.shape
        render = torch.empty(B, C1 - 1, H, W, dtype=torch.float32, device=acc.device)
        existing = torch.empty(B, 1, H, W, dtype=torch.float32, device=acc.device)
        self._call('kbe_normalize', _ptr(_f32c(acc)), B, C1 - 1, W, H, _ptr(render), _ptr(existing), _stream())
        return render, existing

    def render_pointcloud(self, points, data, W, H, focal, baseline, tiled=None):
        """common.py:428-686 -> (render [B,C,H,W], existing [B,1,H,W]).  ``tiled`` (default: env KBE_RENDER_TILED, on):
        one sample at a time through the tile machinery of the frame loop (no float atomics; 20x faster at 68
        channels); off: the stage-by-stage global-atomic kernels (kept as the independent cross-check)."""
        points, data = _f32c(points), _f32c(data)
        B, C, N = data.shape
        dev = points.device
        if tiled is None:
            # the tile renderer's size limits (include/kbe.h); beyond them the stage-by-stage HIP kernels take over
            tiled = (os.environ.get('KBE_RENDER_TILED', '1') != '0' and N <= (1 << 30) and int(W) * int(H) <= (1 << 30)
                     and int(W) < (1 << 23) and int(H) < (1 << 23))
        if tiled:
            W, H = int(W), int(H)
            key = (dev, W, H)
            scratch = self._tiled_scratch.get(key)
            if scratch is None:
                scratch = torch.empty(int(self.lib.kbe_frame_scratch_bytes(W, H, 0)), dtype=torch.uint8, device=dev)
                self._call('kbe_frame_scratch_init', _ptr(scratch, torch.uint8), W, H, _stream())
                self._tiled_scratch = {key: scratch}           # one size at a time (200 MB at 1024^2)
            render = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
            existing = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
            for b in range(B):
                self._call('kbe_render_pointcloud_tiled', _ptr(points[b]), _ptr(data[b]), N, C, W, H, float(focal), float(baseline), None,
                           _ptr(scratch, torch.uint8), _ptr(render[b]), _ptr(existing[b]), _stream())
            return render, existing
        zkeys = torch.empty(B * H * W, dtype=torch.int32, device=dev)
        zee = torch.empty(B * H * W, dtype=torch.float32, device=dev)
        acc = torch.empty(B * (C + 1) * H * W, dtype=torch.float32, device=dev)
        render = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        existing = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
        self._call('kbe_render_pointcloud', _ptr(points), _ptr(data), B, N, C, W, H, float(focal), float(baseline), _ptr(zkeys, torch.int32),
                   _ptr(zee), _ptr(acc), _ptr(render), _ptr(existing), _stream())
        return render, existing

    # -- fill ---------------------------------------------------------------------------
    def fill_disocclusion(self, x, depth):
        x, depth = _f32c(x), _f32c(depth)
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        self._call('kbe_fill_disocclusion', _ptr(x), _ptr(depth), B, C, W, H, _ptr(out), _stream())
        return out

    # -- the frame loop on the resident cloud ---------------------------------------------
    def prepare_cloud(self, points, image, depth, W, H, focal=None, raster=None, near_depth=None):
        """Makes tensorInpaPoints/Image/Depth resident for the frame loop: contiguous fp32 views (used in
        place, no repacking) plus the per-view scratch (z-buffer, tile buckets, hole list), initialised
        once.  Returns the state render_frame consumes."""
        W, H = int(W), int(H)
        N = points.shape[-1]
        dev = points.device
        state = {'points': _f32c(points).reshape(3, N), 'image': _f32c(image).reshape(3, N), 'depth': _f32c(depth).reshape(N),
                 'N': N, 'W': W, 'H': H, 'frame': torch.empty(H, W, 3, dtype=torch.uint8, device=dev),
                 # layout hint: process_kenburns' cloud starts with the W x H image raster (common.py:176-179)
                 'raster_w': W if N >= W * H else 0, 'raster_n': W * H if N >= W * H else 0}
        if raster is not None:          # (width, count): the cloud starts with a row-major raster of another shape
            state['raster_w'], state['raster_n'] = int(raster[0]), int(raster[1])
        if os.environ.get('KBE_NO_RASTER_HINT'):
            state['raster_w'] = state['raster_n'] = 0
        # one scratch per lane of the frame loop (render_video renders consecutive frames on `lanes` streams);
        # render_frame uses lane 0's
        lanes = max(1, min(MAX_LANES, int(os.environ.get('KBE_LANES', DEFAULT_LANES))))
        stride = int(self.lib.kbe_video_scratch_stride(W, H, N))
        state['lanes'] = lanes
        state['scratch'] = torch.empty(lanes * stride, dtype=torch.uint8, device=dev)
        self._call('kbe_frame_scratch_init_sets', state['scratch'].data_ptr(), stride, lanes, W, H, _stream())
        # Two routes for the scatter of a frame, same results (tests/test_hip_parity.py::test_fused_scatter_equals_the_bucket_path):
        #   fused   k_place -> k_frame on the packed cloud (kbe_cloud_pack, once per cloud): every point projected once, its
        #           12-byte placement stored in place, a tile pulls the sub-blocks listed for it, z-tile in LDS; no per-point
        #           global atomic, 1.4x the algorithmic HBM bytes;
        #   bucket  k_project -> k_tiles: 16-byte records appended to per-tile buckets, z-buffer in HBM: 2.0x the bytes.
        # Measured, us per frame left in HBM, bucket / fused: 1024^2 inpainted cloud 29.4 / 25.3, raw 37.4 / 35.5, 2048^2 raw
        # 144 / 122, 512^2 9.3 / 9.1, 256^2 4.3 / 4.5 -- but clouds much denser than the raster pile more records on a tile
        # than its LDS holds and the fused route's further rounds go through HBM: 2048^2 from 16.8 M points 375 / 403, and a
        # dolly zoom-out (the image shrinks, the density grows along the video) 97 / 151.  KBE_FUSED = auto (default: fused
        # unless the cloud has more than 1.5 points per pixel; render_video also looks at the camera path) | 1 | 0.
        mode = os.environ.get('KBE_FUSED', 'auto')
        state['fused'] = ((N <= FUSED_MAX_DENSITY * W * H) if mode == 'auto' else mode not in ('0', 'generic')) and N <= FUSED_MAX_POINTS
        # ... and a third, on request only (KBE_FUSED=generic): the reference's own decomposition (z-splat, degrid, accumulate with global
        # atomics, normalise, fill), one frame at a time -- the independent cross-check of the two tile routes as a whole video loop.  (For a
        # day of round 5 clouds beyond 6.5 points per pixel took it, as the lesser evil next to the tile routes' cliff; with the cliff gone it
        # is 15-35 x slower than the fused route at every density measured.)
        state['generic'] = mode == 'generic'
        state['cloud_focal'] = float(focal) if focal else 512.0
        # the depth of the nearest point (the reference's objectDepthrange[0], common.py:88, when the caller has it; else found
        # on first need): decides how many consecutive frames of a video share candidate lists (include/kbe.h: near_depth)
        state['near_depth'] = None if near_depth is None else (float(near_depth) if 0.0 < float(near_depth) < 1.0e30 else 0.0)     # (nan, inf, <= 0: unknown)
        if state['fused']:
            self._pack(state)
        return state

    @staticmethod
    def near_depth(state):
        """The nearest depth of the cloud, for kbe_render_video / kbe_render_frame_group_ahead's `near_depth` (KBE_SHARE_LISTS=0: 0.0,
        every frame keeps candidate lists of its own).  Found with one reduction and one host synchronisation where the caller of
        prepare_cloud did not pass it."""
        if os.environ.get('KBE_SHARE_LISTS') == '0':
            return 0.0
        if state.get('near_depth') is None:
            z = state['points'][2]
            z = z[z > 0]
            near = float(z.min()) if z.numel() else 0.0
            state['near_depth'] = near if 0.0 < near < 1.0e30 else 0.0
        return state['near_depth']

    def _pack(self, state):
        """kbe_cloud_pack, once per cloud (on first use of the fused route)."""
        if 'packed' not in state:
            N, W, H = state['N'], state['W'], state['H']
            state['packed'] = torch.empty(int(self.lib.kbe_cloud_pack_bytes(N)), dtype=torch.uint8, device=state['points'].device)
            self._call('kbe_cloud_pack', _ptr(state['points']), _ptr(state['image']), _ptr(state['depth']), N, W, H, state['cloud_focal'],
                       state['raster_w'], state['raster_n'], _ptr(state['packed'], torch.uint8), _stream())

    def render_frame(self, state, shift3, focal, baseline, render_f32=None, existing_f32=None, zee_f32=None,
                     zee_pre_f32=None, out=None, stages=7, fill_rect=None, fused=None, parity=-1):
        """One frame of common.py:238-255 (shift -> render -> fill -> uint8) -> uint8 [H,W,3] on the device.
        fill_rect = (x0, y0, x1, y1): only holes inside are filled (see include/kbe.h).  ``fused`` (default: the
        state's route): the one-launch scatter on the packed cloud; False: the bucket path (k_project + k_tiles).
        ``stages``: bit 1 = projection launch (bucket path only), 2 = scatter / tile launch, 4 = hole fill (+ flags).
        ``parity`` (fused route, include/kbe.h): -1 = a frame on its own; 0, 1, 0, ... for consecutive frames on one scratch."""
        frame = state['frame'] if out is None else out
        rect = _rect(fill_rect)
        if state.get('fused') if fused is None else fused:
            self._pack(state)
            self._call('kbe_render_frame_fused', _ptr(state['packed'], torch.uint8), state['N'], state['cloud_focal'], state['W'], state['H'],
                       float(focal), float(baseline), _shift(shift3), _ptr(state['scratch'], torch.uint8), _ptr(frame, torch.uint8), _ptr(render_f32),
                       _ptr(existing_f32), _ptr(zee_f32), _ptr(zee_pre_f32), (int(stages) & ~KBE_STAGE_PROJECT) | fused_build_bits(), rect,
                       int(parity), _stream())
            return frame
        self._call('kbe_render_frame_stages', _ptr(state['points']), _ptr(state['image']), _ptr(state['depth']), state['N'], state['W'], state['H'],
                   float(focal), float(baseline), _shift(shift3), _ptr(state['scratch'], torch.uint8), _ptr(frame, torch.uint8), _ptr(render_f32),
                   _ptr(existing_f32), _ptr(zee_f32), _ptr(zee_pre_f32), int(stages), rect, state['raster_w'], state['raster_n'], _stream(),
                   what='kbe_render_frame')
        return frame

    def group_scratch(self, state, sets):
        """`sets` initialised scratch sets for launches that take several frames (kbe_render_frame_group, KBE_VIDEO_FILL_GROUP),
        allocated on first use: (tensor, stride in bytes)."""
        stride = self.scratch_stride(state)
        if 'scratch_groups' not in state or state['scratch_groups'].numel() < sets * stride:
            state['scratch_groups'] = torch.empty(sets * stride, dtype=torch.uint8, device=state['points'].device)
            self._call('kbe_frame_scratch_init_sets', state['scratch_groups'].data_ptr(), stride, sets, state['W'], state['H'], _stream())
        return state['scratch_groups'], stride

    def _group_sets(self, state, *counts):
        """group_scratch for groups of `counts` frames that keeps the sets already held (four on first use)."""
        held = state['scratch_groups'].numel() // self.scratch_stride(state) if 'scratch_groups' in state else 4
        return self.group_scratch(state, max(*counts, held))

    def render_frame_group(self, state, cameras, baseline, out, stages=7, zbuf_flags=None, fill_rect=None):
        """kbe_render_frame_group: the launches of 1..4 frames [(focal, shift3)] of the bucket route, every launch taking all of
        them; out: uint8 [n,H,W,3] on the device.  Each frame uses a scratch set of its own (state['scratch_groups'])."""
        n = len(cameras)
        scratch, stride = self.group_scratch(state, max(n, 4))
        focals, shifts, sets, frames, rect = _group_args(cameras, scratch, stride, out, fill_rect)
        zf = None if zbuf_flags is None else (ctypes.c_int * n)(*[int(v) for v in zbuf_flags])
        self._call('kbe_render_frame_group', _ptr(state['points']), _ptr(state['image']), _ptr(state['depth']), state['N'], state['W'], state['H'],
                   float(baseline), n, focals, shifts, sets, frames, zf, int(stages), rect, state['raster_w'], state['raster_n'], _stream())
        return out

    def render_frame_group_fused(self, state, cameras, baseline, out, stages=6, parities=None, fill_rect=None):
        """kbe_render_frame_group_fused: the same on the packed cloud (k_place + k_frame + fill, each taking all the frames)."""
        n = len(cameras)
        self._pack(state)
        scratch, stride = self._group_sets(state, n)
        focals, shifts, sets, frames, rect = _group_args(cameras, scratch, stride, out, fill_rect)
        par = None if parities is None else (ctypes.c_int * n)(*[int(v) for v in parities])
        self._call('kbe_render_frame_group_fused', _ptr(state['packed'], torch.uint8), state['N'], state['cloud_focal'], state['W'], state['H'],
                   float(baseline), n, focals, shifts, sets, frames, par, int(stages) | fused_build_bits(), rect, _stream())
        return out

    def render_frame_group_ahead(self, state, cameras, baseline, out, turn, placed, next_cameras=None, stages=6, fill_rect=None, next_turn=None):
        """kbe_render_frame_group_ahead: frame k on scratch set k of the group scratch, on the set's turn `turn` (an int for all, or
        one per frame); the tile launch makes the placements of `next_cameras` when given (frame k on set k, turn `next_turn`:
        default turn + 1)."""
        n = len(cameras)
        m = len(next_cameras) if next_cameras else 0
        self._pack(state)
        scratch, stride = self._group_sets(state, n, m)
        focals, shifts, sets, frames, rect = _group_args(cameras, scratch, stride, out, fill_rect)
        nf, ns, nsets = _group_args(next_cameras, scratch, stride)[:3] if m else (None, None, None)
        turn = [int(turn)] * n if isinstance(turn, int) else [int(t) for t in turn]
        if next_turn is None:
            next_turn = [(turn[k] if k < n else turn[0]) + 1 for k in range(m)]
        turns = (ctypes.c_int * n)(*turn)
        nturns = (ctypes.c_int * m)(*[int(t) for t in next_turn]) if m else None
        self._call('kbe_render_frame_group_ahead', _ptr(state['packed'], torch.uint8), state['N'], state['cloud_focal'], state['W'], state['H'],
                   float(baseline), n, focals, shifts, sets, frames, turns, 1 if placed else 0, m, nf, ns, nsets, nturns,
                   int(stages) | fused_build_bits(), rect, self.near_depth(state), _stream())
        return out

    def prepared_group_ahead(self, state, cameras, baseline, out, next_cameras, stages=2):
        """A closure that makes the launch of :meth:`render_frame_group_ahead` for a FIXED group -- frame k on scratch set k, the next
        group the same sets -- with every argument array built once: ``launch(turn, placed, place_next=True)`` only writes the turn
        numbers.  For timing loops: building the ctypes arrays of two groups of eight cameras costs the host about as long as the
        GPU works on the launch, and a measurement through the ordinary wrapper then reads the host's speed."""
        n, m = len(cameras), len(next_cameras)
        self._pack(state)
        scratch, stride = self._group_sets(state, n, m)
        focals, shifts, sets, frames, _ = _group_args(cameras, scratch, stride, out)
        nf, ns, nsets = _group_args(next_cameras, scratch, stride)[:3]
        turns, nturns = (ctypes.c_int * n)(), (ctypes.c_int * m)()
        fixed = (_ptr(state['packed'], torch.uint8), state['N'], state['cloud_focal'], state['W'], state['H'], float(baseline), n,
                 focals, shifts, sets, frames, turns)
        tail = (nf, ns, nsets, nturns, int(stages) | fused_build_bits(), None, self.near_depth(state))
        fn, check = self.lib.kbe_render_frame_group_ahead, self._check
        assert len(fixed) + 2 + len(tail) + 1 == len(prototypes()['kbe_render_frame_group_ahead'][1])       # (launch passes: fixed, placed, n_next, tail, stream)
        keep = (scratch, out)          # (the arrays hold raw addresses)

        def launch(turn, placed, place_next=True):
            for k in range(n):
                turns[k] = turn
            for k in range(m):
                nturns[k] = turn + 1
            check(fn(*fixed, 1 if placed else 0, m if place_next else 0, *tail, _stream()), 'kbe_render_frame_group_ahead')
        launch.keep = keep
        return launch

    def scratch_stride(self, state):
        """Bytes between two scratch sets of the cloud's frame size (kbe_video_scratch_stride), asked once per cloud."""
        if 'scratch_stride' not in state:
            state['scratch_stride'] = int(self.lib.kbe_video_scratch_stride(state['W'], state['H'], state['N']))
        return state['scratch_stride']

    def scratch_set_budget(self, state, budget_mb=None):
        """How many scratch sets (kbe_video_scratch_stride bytes each) a video loop may hold: `budget_mb` (KBE_SCRATCH_BUDGET_MB), or half
        of the device memory that is free now plus what the cloud's sets already hold; at least one per lane."""
        stride = self.scratch_stride(state)
        if budget_mb is not None:
            budget = budget_mb * 1e6
        else:
            free, _ = torch.cuda.mem_get_info(state['points'].device)
            held = state['scratch_groups'].numel() if 'scratch_groups' in state else 0
            budget = 0.5 * (free + held)
        return max(state['lanes'], int(budget // stride))

    def video_launch_shape(self, state, cameras, batch, to_host=False, max_group=None):
        """(flags of kbe_render_video, frames per launch, fused route?) for a video of `cameras`, under the environment's switches: the
        group-and-fill rule of video_shape (fills_with_tables, frames_per_launch -- the measurements are there), of which
        video_shape.call_shape makes a whole call.  `flags` holds KBE_VIDEO_FILL_DIST and the group field only."""
        sw = video_switches()
        N, W, H, fused = state['N'], state['W'], state['H'], bool(state.get('fused'))
        fill_dist = video_shape.fills_with_tables(N, W, H, HipKernels.zooms_out(state, cameras), sw)
        group = video_shape.frames_per_launch(N, W, H, fused, fill_dist, batch, to_host, sw)
        if max_group is not None:
            group = max(1, min(group, int(max_group)))
        return video_shape.launch_flags(fill_dist, group), group, fused

    @staticmethod
    def zooms_out(state, cameras):
        return bool(cameras) and min(float(c[0]) for c in cameras) < 0.9 * state['cloud_focal']

    def delivery_lanes(self, state, cameras, baseline, crop=None, switches=None):
        """Lanes of the frame loop when the frames go to pinned host memory: two where the link binds, all where the rendering
        does (`host_lanes` has the measurements).  Which it is depends on the cloud, the camera path and the route, so it is
        MEASURED once per cloud, camera-path kind and crop -- twelve of the video's frames rendered into HBM on all lanes, timed
        with two events (a few hundred microseconds, and ONE host synchronisation: the first render_video of a cloud is not
        enqueue-only) -- and kept in the cloud's state; videos shorter than PROBE_MIN_FRAMES (the product's 75 frames: the probe would
        be a third of their work), and the first lookup without a camera path, take the a-priori estimate.  A rank that received the cloud by broadcast takes what rank 0 measured (`delivery_lanes_hint`:
        sharding.measure_delivery_lanes) and never probes.  Env KBE_HOST_LANES overrides (`switches`: render_video's record, which has read it already)."""
        lanes, W, H = state['lanes'], state['W'], state['H']
        forced = forced_host_lanes() if switches is None else switches.host_lanes
        if forced is not None:
            return min(lanes, max(1, forced))
        zoom = self.zooms_out(state, cameras)                  # a zoom-out renders differently: its own entry
        hint = state.get('delivery_lanes_hint', {})
        if zoom in hint:                                       # measured on rank 0, broadcast with the cloud (sharding.py)
            return min(lanes, max(1, int(hint[zoom])))
        key = (zoom, None if crop is None else (int(crop[0]), int(crop[1])))
        cache = state.setdefault('delivery_lanes', {})
        if key in cache:
            return cache[key]
        # (a video shorter than PROBE_MIN_FRAMES takes the a-priori estimate: the probe renders 24 frames and synchronises the host --
        # 0.5 ms of the 1.4 ms a 64-frame 512^2 video takes, paid by every Pipeline call, each with a cloud of its own: ADVICE r3)
        if len(cameras) < PROBE_MIN_FRAMES or lanes == 1:
            return video_shape.host_lanes(lanes, state['N'], W, H, 3 * W * H)
        probe = cameras[::max(1, len(cameras) // 12)][:12]
        out = torch.empty(len(probe), H, W, 3, dtype=torch.uint8, device=state['points'].device)
        self.render_video(state, probe, baseline, crop=crop, host_out=out)                          # warm-up: scratch, streams, the packed cloud
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.render_video(state, probe, baseline, crop=crop, host_out=out)
        e1.record()
        e1.synchronize()
        render_us = e0.elapsed_time(e1) * 1e3 / len(probe)
        cache[key] = lanes_for_delivery(lanes, render_us, 3 * W * H)       # a cropped frame is resized back to W x H (common.py:257)
        state['delivery_probe_us'] = render_us
        return cache[key]

    def _render_video_generic(self, state, cameras, baseline, crop, host_out):
        """The frame loop on the stage-by-stage kernels (kbe_shift_points, kbe_render_pointcloud's z-splat / degrid / accumulate /
        normalise with global atomics, kbe_fill_disocclusion, kbe_frame_u8, kbe_crop_resize_u8) -- the reference's own decomposition
        of common.py:238-257 (KBE_FUSED=generic: a cross-check of the tile routes, not a product route).  Frame by frame from Python:
        at >= 1 ms of GPU work per frame the loop's own cost does not matter."""
        n, W, H = len(cameras), state['W'], state['H']
        dev = state['points'].device
        if 'generic_data' not in state:
            state['generic_data'] = torch.cat([state['image'], state['depth'].reshape(1, -1)], 0).unsqueeze(0).contiguous()      # [1,4,N]: image; depth
        pts0, data = state['points'].unsqueeze(0), state['generic_data']
        out = host_out if host_out.is_cuda else torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        for i, (focal, shift3) in enumerate(cameras):
            pts = self.shift_points(pts0, shift3)                                                           # common.py:104-109
            render, existing = self.render_pointcloud(pts, data, W, H, focal, baseline, tiled=False)        # :428-686
            render = self.fill_disocclusion(render, render[:, 3:4] * (existing > 0.0).float())              # :253
            frame = self.frame_u8(render[:, 0:3])                                                           # :255
            out[i].copy_(frame if crop is None else self.crop_resize_u8(frame, int(crop[0]), int(crop[1])))  # :256-257
        if not host_out.is_cuda:
            host_out[:n].copy_(out, non_blocking=True)
        return host_out

    def render_video(self, state, cameras, baseline, crop=None, host_out=None, overlap=True, batch=None):
        """The frame loop for a list of (focal, shift3) cameras, enqueued natively; returns the pinned host
        tensor [n,H,W,3] the frames land in (valid after the current stream is synchronised).  ``host_out`` may
        also be a DEVICE tensor: the frames then stay in HBM (the last kernel of every frame stores straight into
        it, no transfer).  ``batch`` selects the hand-off to host memory (None: groups of up to 32 frames per
        transfer on KBE_HOST_LANES lanes; see include/kbe.h); ``overlap`` only matters for ``batch`` > 0."""
        n, W, H = len(cameras), state['W'], state['H']
        dev = state['points'].device
        if host_out is None:
            host_out = torch.empty(n, H, W, 3, dtype=torch.uint8, pin_memory=True)
        assert host_out.dtype == torch.uint8 and host_out.is_contiguous() and host_out.numel() >= n * H * W * 3
        if state.get('generic'):
            if not host_out.is_cuda and not host_out.is_pinned():
                raise KbeError('render_video: host_out must be pinned host memory (or a device tensor)')
            return self._render_video_generic(state, cameras, baseline, crop, host_out)
        to_host = not host_out.is_cuda
        if to_host and not host_out.is_pinned():
            raise KbeError('render_video: host_out must be pinned host memory (or a device tensor)')
        sw = video_switches()
        lanes = self.delivery_lanes(state, cameras, baseline, crop, sw) if to_host else state['lanes']
        held = state['scratch_groups'].numel() // self.scratch_stride(state) if 'scratch_groups' in state else 0
        shape = video_shape.call_shape(state['N'], W, H, bool(state.get('fused')), n, self.zooms_out(state, cameras), to_host, batch, lanes, sw,
                                       held, lambda: self.scratch_set_budget(state, sw.scratch_budget_mb))
        batch, fused = shape.batch, shape.fused
        need = int(self.lib.kbe_video_stage_bytes(W, H, lanes, batch))
        if 'stage' not in state or state['stage'].numel() < need:
            state['stage'] = torch.empty(need, dtype=torch.uint8, device=dev)
        if 'copy_stream' not in state:
            state['copy_stream'] = torch.cuda.Stream(device=dev)
            state['lane_streams'] = [None] + lane_streams_of(dev, state['lanes'] - 1)
        lane_streams = (ctypes.c_void_p * MAX_LANES)(*[None if st is None else st.cuda_stream for st in state['lane_streams']])
        focals = (ctypes.c_double * max(n, 1))(*[float(c[0]) for c in cameras])
        shifts = (ctypes.c_float * max(3 * n, 1))(*[float(v) for c in cameras for v in c[1]])
        cw, ch = (0, 0) if crop is None else (int(crop[0]), int(crop[1]))
        copy_stream = state['copy_stream'].cuda_stream if overlap and to_host else _stream()
        if fused:
            self._pack(state)
        # one frame per launch renders on the lanes' own sets, more on the group scratch (shape.group sets per lane, allocated on first use)
        state['video_sets'] = shape.sets
        scratch = self.group_scratch(state, shape.sets)[0] if shape.group > 1 else state['scratch']
        self._call('kbe_render_video', _ptr(state['points']), _ptr(state['image']), _ptr(state['depth']), state['N'], W, H, float(baseline), n,
                   focals, shifts, cw, ch, _ptr(scratch, torch.uint8), _ptr(state['stage'], torch.uint8), batch, host_out.data_ptr(),
                   state['raster_w'], state['raster_n'], _ptr(state['packed'], torch.uint8) if fused else None, state['cloud_focal'], shape.flags,
                   _stream(), copy_stream, lanes, lane_streams, self.near_depth(state) if fused else 0.0)
        return host_out

    def handoff_status(self):
        """After synchronising a delivered video's stream: raises KbeError when an SDMA hand-off of this process gave up waiting for its
        engine (kbe_video_handoff_status: the frames of that video are not all in host memory)."""
        self._call('kbe_video_handoff_status')

    def generate_mask_raw(self, points, shift, W, H, focal, baseline, want_tables=False):
        """generate_mask's kernel (common.py:696-817) -> masks [B,1,N] (and zee [B,1,H,W], ids [B,H,W] int32)."""
        points = _f32c(points)
        B, _, N = points.shape
        dev = points.device
        shift = _f32c(shift).reshape(B, 3).to(dev)
        keys = torch.empty(B * H * W, dtype=torch.int64, device=dev)
        winner = torch.empty(B, max(N, 1), dtype=torch.int32, device=dev)
        masks = torch.empty(B, 1, N, dtype=torch.float32, device=dev)
        zee = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev) if want_tables else None
        ids = torch.empty(B, H, W, dtype=torch.int32, device=dev) if want_tables else None
        self._call('kbe_generate_mask', _ptr(points), _ptr(shift), B, N, int(W), int(H), float(focal), float(baseline), _ptr(keys, torch.int64),
                   _ptr(winner, torch.int32), _ptr(masks), _ptr(zee), _ptr(ids, torch.int32), _stream())
        return (masks, zee, ids) if want_tables else masks

    def generate_mask(self, points, shift, W, H, focal, baseline):
        """common.py:689-830: the ownership mask as an image (N == H*W), median-5 filtered (:829)."""
        masks = self.generate_mask_raw(points, shift, W, H, focal, baseline)
        return self.spatial_filter(masks.view(-1, 1, int(H), int(W)), 'median-5')

    def zkeys_clear(self, zkeys):
        self._call('kbe_zkeys_clear', _ptr(zkeys, torch.int32), zkeys.numel(), _stream())

    def frame_u8(self, render):
        render = _f32c(render)
        _, C, H, W = render.shape
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=render.device)
        self._call('kbe_frame_u8', _ptr(render), W, H, _ptr(out, torch.uint8), _stream())
        return out

    def crop_resize_u8(self, frame, crop_w, crop_h):
        H, W, _ = frame.shape
        out = torch.empty_like(frame)
        self._call('kbe_crop_resize_u8', _ptr(frame, torch.uint8), W, H, int(crop_w), int(crop_h), _ptr(out, torch.uint8), _stream())
        return out

    # -- Motion-JPEG and PNG on the device -----------------------------------------------
    def encode_raw(self, fmt, pointers, n, W, H, stride, own, scratch, out, cap, offsets, status):
        """kbe_<fmt>_encode as it is (include/kbe.h, the encoders' common contract), on the current stream: addresses, not tensors; `own`: the
        entry's integers between the stride and the scratch (the quality, the flags).  -> its return code."""
        return self._raw('kbe_%s_encode' % fmt, pointers, n, W, H, stride, *own, scratch, out, cap, offsets, status, _stream())

    def mjpeg_encode(self, frames, quality=92, bgr=False, cap=None):
        """uint8 [n,H,W,3] frames in HBM -> one baseline JPEG (bytes) per frame, encoded on the device (kbe_mjpeg_encode): the streams
        come to the host, not the pixels.  ``bgr``: the frames hold B, G, R (what Pipeline renders from a cv2.imread image).  One
        synchronisation for the offsets and the status word, then exactly offsets[n] bytes are copied.  ``cap``: the stream buffer's
        size (default: a quarter of the raw frames -- photographs at quality 92 take about a tenth); when the streams do not fit,
        the call is repeated once with a buffer of the true size, which the first run has reported."""
        quality, flags = int(quality), KBE_MJPEG_BGR if bgr else 0
        return encode_units('mjpeg_encode', 'kbe_mjpeg_encode', frames, self.lib.kbe_mjpeg_scratch_bytes, cap, lambda n, step: n * (1024 + step // 4),
                            lambda pointers, n, W, H, stride, scratch, out, cap, offsets, status, stream:
                            self._call('kbe_mjpeg_encode', pointers, n, W, H, stride, quality, flags, scratch, out, cap, offsets, status, stream))

    def png_encode(self, frames, bgr=False, cap=None):
        """uint8 [n,H,W,3] frames in HBM -> one PNG file (bytes) per frame, encoded on the device (kbe_png_encode): lossless, a file decodes
        to its frame.  ``bgr``: the frames hold B, G, R (what Pipeline renders from a cv2.imread image); the files hold R, G, B either way.
        One synchronisation for the offsets and the status word, then exactly offsets[n] bytes are copied.  ``cap``: the files' buffer
        (default: the raw size of the frames plus a kilobyte per frame -- only noise needs more); when the files do not fit, the call is
        repeated once with a buffer of the true size, which the first run has reported."""
        flags = KBE_PNG_BGR if bgr else 0
        return encode_units('png_encode', 'kbe_png_encode', frames, self.lib.kbe_png_scratch_bytes, cap, lambda n, step: n * (1024 + step),
                            lambda pointers, n, W, H, stride, scratch, out, cap, offsets, status, stream:
                            self._call('kbe_png_encode', pointers, n, W, H, stride, flags, scratch, out, cap, offsets, status, stream))

    # -- torch glue ---------------------------------------------------------------------
    def depth_to_points(self, depth, focal, valid=None):
        depth = _f32c(depth)
        B, _, H, W = depth.shape
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=depth.device)
        self._call('kbe_depth_to_points', _ptr(depth), _ptr(None if valid is None else _f32c(valid)), B, W, H, float(focal), _ptr(out), _stream())
        return out

    def shift_points(self, points, shift3):
        points = _f32c(points)
        B, _, N = points.shape
        out = torch.empty_like(points)
        self._call('kbe_shift_points', _ptr(points), B, N, _shift(shift3), _ptr(out), _stream())
        return out

    def spatial_filter(self, x, kind):
        code = {'laplacian': 0, 'median-3': 3, 'median-5': 5}.get(kind)
        if code is None:
            return None       # the reference returns None for unknown types (common.py:395,425)
        x = _f32c(x)
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        self._call('kbe_spatial_filter', _ptr(x), B * C, W, H, code, _ptr(out), _stream())
        return out

    def laplacian_valid(self, disparity, scale, threshold):
        """(|laplacian(disparity / scale)| < threshold).float(); `scale` is a 0-dim device tensor."""
        x = _f32c(disparity)
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        scale = _f32c(scale).reshape(1)
        self._call('kbe_laplacian_valid', _ptr(x), _ptr(scale), B * C, W, H, float(threshold), _ptr(out), _stream())
        return out

    def prelu_mask(self, x, slope, mask=None, out=None):
        """prelu(x, slope) * mask in one pass (kbe_prelu_mask); mask [B,1,H,W] or None."""
        x = _f32c(x)
        B, C, H, W = x.shape
        if mask is not None and tuple(mask.shape) != (B, 1, H, W):
            raise KbeError('prelu_mask: the mask must be [B,1,H,W] = %s, got %s' % ((B, 1, H, W), tuple(mask.shape)))
        out = torch.empty_like(x) if out is None else out
        self._call('kbe_prelu_mask', _ptr(x), _ptr(_f32c(slope)), _ptr(None if mask is None else _f32c(mask)), B, C, H, W, _ptr(out), _stream())
        return out

    def bias_act(self, x, bias=None, slope=None, res1=None, res2=None, out=None):
        """act(x + bias[c]) + res1 + res2 in one pass (kbe_bias_act): x [B,C,H,W] contiguous fp32; every other operand optional.
        `out` may be `x` itself (a convolution's fresh output)."""
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
        B, C, H, W = x.shape
        out = torch.empty_like(x) if out is None else out
        res1, res2 = (None if r is None else _f32c(r) for r in (res1, res2))
        assert all(r is None or r.shape == x.shape for r in (res1, res2))
        self._call('kbe_bias_act', _ptr(x), _ptr(None if bias is None else _f32c(bias)), _ptr(None if slope is None else _f32c(slope)), _ptr(res1),
                   _ptr(res2), B, C, H, W, _ptr(out), _stream())
        return out

    def upsample2x_act(self, x, slope=None):
        """prelu(bilinear x2 upsampling of x, align_corners=False) in one pass (kbe_upsample2x_act); slope [C] or None."""
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
        B, C, H, W = x.shape
        out = torch.empty(B, C, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
        self._call('kbe_upsample2x_act', _ptr(x), _ptr(None if slope is None else _f32c(slope)), B, C, H, W, _ptr(out), _stream())
        return out

    @staticmethod
    def fused_layers_take(shape, upsample=False):
        """Do the fused passes of the plain networks take a [B,C,H,W] tensor -- bias_act as its x, and with ``upsample`` upsample2x_act
        as its input?  Their grids hold a plane in one block row (B C <= 65535) and upsample2x_act an output row in another
        (2 H <= 65535); the entries refuse anything above (include/kbe.h).  The ONE place the callers ask (pointcloud_inpainting._fused_layers,
        _main_fused; partial_inpainting.Upsample.forward): a shape that is not taken runs as the stock modules it would have run without
        the fused passes."""
        B, C, H, _ = shape
        return B * C <= 65535 and (not upsample or 2 * H <= 65535)

    pconv_epilogue_adds_bias = True         # (PartialConv2d.forward: run the convolution without its bias)

    def pconv_epilogue(self, raw, bias, mask, kernel_size, stride, padding, in_channels=None, in_size=None, act_slope=None, residual=None,
                       raw_without_bias=False):
        """raw [B,Cout,Ho,Wo] = conv(x * mask); mask [B,Cin|1,H,W] or None (then in_channels/in_size say what x was).
        act_slope [Cout] / residual [B,Cout,Ho,Wo] (optional): out = prelu(out + residual) in the same pass (include/kbe.h).
        raw_without_bias: the convolution was run without its bias; the epilogue adds it first (same values, one pass less)."""
        raw = _f32c(raw)
        B, Cout, Ho, Wo = raw.shape
        if mask is not None:
            mask = _f32c(mask)
            _, Cm, H, W = mask.shape
            Cin = Cm if in_channels is None else int(in_channels)
        else:
            Cm, Cin, (H, W) = 1, int(in_channels), in_size
        out = torch.empty_like(raw)
        um = torch.empty(B, 1, Ho, Wo, dtype=torch.float32, device=raw.device)
        if residual is not None:
            residual = _f32c(residual)
            assert residual.shape == raw.shape
        self._call('kbe_pconv_epilogue', _ptr(raw), _ptr(None if bias is None else _f32c(bias)), _ptr(mask), Cm, B, Cin, H, W, Cout, Ho, Wo,
                   int(kernel_size), int(stride), int(padding), _ptr(out), _ptr(um), _ptr(None if act_slope is None else _f32c(act_slope)),
                   _ptr(residual), 1 if raw_without_bias and bias is not None else 0, _stream())
        return out, um


class HipSerialScheduleKernels:
    """KBE_DEGRID=serial: the frames the REFERENCE-RUN fixtures hold (tests/golden/kenburns_*.npz: the reference's kernel text
    executed one element after the other), from the HIP library.

    The reference's updateDegrid (common.py:525-568) rewrites the z-buffer in place while its neighbours read it; what a CUDA
    run produces lies somewhere between the serial index order and the out-of-place (Jacobi) schedule and is not reproducible
    from run to run.  The product's default is Jacobi -- the fused tile launch, the only deterministic
    parallel schedule: against the serial one it moves 0.1-0.65 % of a frame's pixels (32-59 dB by scene).  This kernel set is the
    other end of that range: every op is still the HIP library's, but render_pointcloud / render_frame run stage by stage --
    kbe_zsplat, kbe_degrid_serial (a wavefront sweep with exactly the serial schedule's data dependences), kbe_accumulate,
    kbe_normalize, kbe_fill_disocclusion, kbe_frame_u8 -- one frame at a time (no native video loop).  Byte for byte the frames
    of the fixtures up to the order of the fp32 atomics (one count on < 0.2 % of the values); ~2 ms per 1024^2 frame instead
    of 21 us: for comparisons with a serial execution of the reference, not for production."""
    name = 'hip-serial'

    def __init__(self, K, keep_zee=False):
        self.K, self.zee_log = K, ([] if keep_zee else None)

    def __getattr__(self, name):
        if name == 'render_video':            # forces common.render_frames onto the per-frame loop below
            raise AttributeError(name)
        return getattr(self.K, name)

    def render_pointcloud(self, points, data, W, H, focal, baseline):
        zkeys, _ = self.K.zsplat(points, W, H, focal, baseline)                                     # common.py:435-507
        zee = self.K.degrid_serial(zkeys=zkeys)                                                     # :525-568, serial schedule
        if self.zee_log is not None:
            self.zee_log.append(zee)
        return self.K.normalize(self.K.accumulate(points, data, zee, focal, baseline))              # :586-669, :686

    def prepare_cloud(self, points, image, depth, W, H, focal=None, raster=None, **kw):
        return {'points': points.reshape(1, 3, -1), 'data': torch.cat([image.reshape(1, 3, -1), depth.reshape(1, 1, -1)], 1), 'W': W, 'H': H}

    def render_frame(self, state, shift3, focal, baseline, fill_rect=None, **kw):
        pts = self.K.shift_points(state['points'], shift3)                                          # common.py:238-244
        render, existing = self.render_pointcloud(pts, state['data'], state['W'], state['H'], focal, baseline)   # :246-251
        filled = self.K.fill_disocclusion(render, render[:, 3:4] * (existing > 0.0).float())       # :253
        return self.K.frame_u8(filled)                                                              # :255


_kernels = None
_serial_kernels = None


def degrid_schedule():
    """KBE_DEGRID=jacobi (default: the fused tile launch) | serial (HipSerialScheduleKernels)."""
    v = os.environ.get('KBE_DEGRID', 'jacobi')
    if v not in ('jacobi', 'serial'):
        raise KbeError('KBE_DEGRID=%r: jacobi (default) or serial' % v)
    return v


def kernels():
    """The process-wide kernel set (HIP).  Raises KbeError when the extension is missing.  KBE_DEGRID=serial: the same library
    behind HipSerialScheduleKernels (read per call, like every other switch of the host side)."""
    global _kernels, _serial_kernels
    if _kernels is None:
        _kernels = HipKernels()
    if degrid_schedule() == 'serial':
        if _serial_kernels is None:
            _serial_kernels = HipSerialScheduleKernels(_kernels)
        return _serial_kernels
    return _kernels
