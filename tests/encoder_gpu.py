"""What the GPU tests of the device-side encoders share (kbe_mjpeg_encode and kbe_png_encode of include/kbe.h, kbe_gif_encode of include/kbe_gif.h:
one contract, csrc/kbe_units_scan.h): one descriptor per encoder, the harness that calls an entry through its typed binding with sentinels
around everything it may write, smoke()'s scene, and a Pipeline without its models.  tests/test_encoders_gpu.py holds the contract against all
three; test_mjpeg_gpu.py, test_png_gpu.py and test_gif_gpu.py what is one format's own."""
import collections
import ctypes
import functools

import numpy as np
import torch

import gif_cases as gc
import mjpeg_cases as mc
import png_cases as pc
from guarded import GUARD, SENTINEL, Guard           # (0xA5, 4096: the bands of the output buffer here are the harness's)


def kernels():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def gif():
    from ken_burns_effect_amd import gif as module
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    module.load()
    return module


def stream():
    from ken_burns_effect_amd import _native
    return _native._stream()


current_stream = stream            # (run takes a `stream` of its own)


def on_device(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.array(a)).cuda()           # (a copy: the cases' arrays are read-only)


@functools.lru_cache(maxsize=None)
def gif_lut(name, flags=0):
    """A GIF case's cell -> index table on the device, kept for the life of the process: the entry takes its address."""
    return on_device(gc.case_palette(name, flags)[1])


# fmt: kbe_<fmt>_encode, kbe_<fmt>_scratch_bytes, kbe_<fmt>_bound; cases: the CPU suite's module (CASES, case_frames, case_twin, BGR); sized: the name
# of the suite's photograph of a size ('17x16'); names: the entry's own arguments, by the header's names, between stride_bytes and scratch;
# own(name, flags): their values for a case (the GIF's: no dither, 4 cs, the case's table); via(K): (the _raw that calls the entry, the typed
# library for its sizes); encode(K, frames, name, **kw): the tensor-level call; ladder: the case of the too-small-buffer test; refused: what the
# entry refuses of its own, as changes to a good call's arguments
Encoder = collections.namedtuple('Encoder', 'fmt cases sized names own via encode ladder refused')
MJPEG = Encoder('mjpeg', mc, 'size_%s', ('quality', 'flags'), lambda name, flags=0: (mc.CASES[name][2], flags), lambda K: (K._raw, K.lib),
                lambda K, frames, name, **kw: K.mjpeg_encode(frames, mc.CASES[name][2], **kw), 'noise',
                {'quality 0': lambda a: a.update(quality=0), 'quality 101': lambda a: a.update(quality=101)})
PNG = Encoder('png', pc, 'size_%s', ('flags',), lambda name, flags=0: (flags,), lambda K: (K._raw, K.lib), lambda K, frames, name, **kw: K.png_encode(frames, **kw), 'photo_like',
              {'a refused size': lambda a: a.update(W=65535, H=65535, stride_bytes=3 * 65535)})         # a file of 2^31 bytes or more
GIF = Encoder('gif', gc, '%s', ('flags', 'dither', 'delay_cs', 'lut'), lambda name, flags=0, dither=0: (flags, dither, 4, gif_lut(name, flags).data_ptr()),
              lambda K: (gif()._raw, gif().load()),
              lambda K, frames, name, bgr=False, **kw: gif().encode(frames, gif_lut(name, gc.BGR if bgr else 0), bgr=bgr, dither='none', **kw), 'photo_like',
              {'null lut': lambda a: a.update(lut=None), 'delay -1': lambda a: a.update(delay_cs=-1), 'delay 65536': lambda a: a.update(delay_cs=65536),
               'dither -1': lambda a: a.update(dither=-1), 'dither 65': lambda a: a.update(dither=65),
               'a refused size': lambda a: a.update(W=65535, H=65535, stride_bytes=3 * 65535)})         # a unit of 2^31 bytes or more
ENCODERS = [MJPEG, PNG, GIF]


def pointers_of(frames, n=None):
    count, H, Wt, _ = frames.shape
    n = count if n is None else n
    return (ctypes.c_void_p * max(n, 1))(*[frames.data_ptr() + i * H * Wt * 3 for i in range(n)])


def run(K, enc, frames, own, cap, W=None, n=None, shift=0, status_before=7, change=None, stream=None):
    """The entry on a uint8 device tensor [n,H,Wt,3] (W <= Wt: the rows' stride is Wt's) with a buffer of `cap` bytes (`shift` bytes off its
    allocation's start) followed by GUARD bytes, everything the call may write filled with sentinels first; own: the values of enc.names.
    The scratch is exactly kbe_<fmt>_scratch_bytes, rounded up only to the 8 bytes its alignment check asks for, every byte of it 0xFF, and
    like the offsets and the status word between two guard bands (tests/guarded.py) that the call must leave alone.  change(args): the last
    word on the argument list -- a dict by the header's names; stream: the kbe_stream_t of the call (default: torch's current stream).
    -> (rc, offsets, status, the buffer with its guard, whether the scratch still holds its poison)."""
    raw, lib = enc.via(K)
    count, H, Wt, _ = frames.shape
    W = Wt if W is None else W
    n = count if n is None else n
    guard = Guard(poison=0xFF)
    good = max(int(getattr(lib, 'kbe_%s_scratch_bytes' % enc.fmt)(W, H, max(n, 1))), 8)
    scratch = guard.empty(((good + 7) // 8 * 8,), torch.uint8, 'cuda')
    out = torch.full((shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    offsets = guard.full((max(n, 1) + 1,), -1, torch.int64, 'cuda')
    status = guard.full((1,), status_before, torch.int32, 'cuda')
    args = dict(frames_u8=pointers_of(frames, n), n_frames=n, W=W, H=H, stride_bytes=3 * Wt, **dict(zip(enc.names, own)), scratch=scratch.data_ptr(),
                out=out.data_ptr() + shift, cap=cap, offsets=offsets.data_ptr(), status=status.data_ptr(), stream=current_stream() if stream is None else stream)
    assert len(own) == len(enc.names)
    if change:
        change(args)
    rc = raw('kbe_%s_encode' % enc.fmt, *args.values())
    torch.cuda.synchronize()
    guard.check()
    got = out.cpu().numpy()
    assert (got[:shift] == SENTINEL).all()
    return rc, offsets.cpu().tolist(), int(status.item()), got[shift:], bool((scratch == 0xFF).all())


def sizes_of(want):
    return np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()


def assert_units(K, enc, frames, own, want, room=333, **kw):
    """The device's streams, files or units of `frames` are `want`, back to back; no byte in front of them or behind them is touched."""
    total = sum(len(s) for s in want)
    rc, offsets, status, buf, _ = run(K, enc, on_device(frames), own, total + room, **kw)
    assert rc == 0 and status == 0
    assert offsets == sizes_of(want)
    assert buf[:total].tobytes() == b''.join(want)
    assert (buf[total:] == SENTINEL).all()


def assert_case(K, enc, name, dithers=((),)):
    """A case of the CPU suite, 1, 3 and 13 frames of different content (13: two launches, the offsets carry on), RGB and BGR; dithers: what
    follows the flags in own() and in case_twin() -- the GIF's dither off and on."""
    dev = on_device(enc.cases.case_frames(name, 13))
    for flags in (0, enc.cases.BGR):
        for dither in dithers:
            want = enc.cases.case_twin(name, 13, flags, *dither)[0]
            for n in (1, 3, 13):
                assert_units(K, enc, dev[:n], enc.own(name, flags, *dither), want[:n])


# what every encoder refuses, as changes to a good call of three 17x16 frames (rows of 16 pixels) by the header's names; an encoder's own: Encoder.refused
REFUSALS = {'null frames': lambda a: a.update(frames_u8=None),
            'null frame 1': lambda a: a['frames_u8'].__setitem__(1, None),
            'n = 0': lambda a: a.update(n_frames=0),
            'n = -3': lambda a: a.update(n_frames=-3),
            'W = 0': lambda a: a.update(W=0),
            'H = 0': lambda a: a.update(H=0),
            'W = 65536': lambda a: a.update(W=65536, stride_bytes=3 * 65536),
            'H = 65536': lambda a: a.update(H=65536),
            'stride < 3 W': lambda a: a.update(stride_bytes=3 * a['W'] - 1),
            'W = 17 in rows of 16': lambda a: a.update(W=17),
            'unknown flag': lambda a: a.update(flags=2),
            'flags = -1': lambda a: a.update(flags=-1),
            'misaligned scratch': lambda a: a.update(scratch=a['scratch'] + 4),
            'null scratch': lambda a: a.update(scratch=None),
            'misaligned offsets': lambda a: a.update(offsets=a['offsets'] + 4),
            'null offsets': lambda a: a.update(offsets=None),
            'null status': lambda a: a.update(status=None),
            'null out with a cap': lambda a: a.update(out=None)}


def refusals_of(enc):
    assert not set(REFUSALS) & set(enc.refused)
    return sorted(set(REFUSALS) | set(enc.refused))


def assert_refused(K, enc, what):
    """KBE_E_INVALID with the entry's name in the text, before anything is enqueued: the offsets, the status word, the buffer and the
    scratch are what they were, and their guard bands too (run)."""
    name = enc.sized % '17x16'
    rc, offsets, status, buf, scratch_untouched = run(K, enc, on_device(enc.cases.case_frames(name, 3)), enc.own(name), 4096, change=REFUSALS.get(what) or enc.refused[what])
    assert rc == -1 and K.lib.kbe_last_error().decode().startswith('kbe_%s_encode: ' % enc.fmt)
    assert offsets == [-1] * 4 and status == 7 and (buf == SENTINEL).all() and scratch_untouched


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


def pipeline_without_models(P, monkeypatch, in_hbm, raw):
    """-> (Stub(output_frames): a Pipeline of the module P without models, whose frame loop hands out the rendered scene -- in HBM when it is
    asked to keep the frames there --, on a machine without ffmpeg; asked: {'keep_on_device': what the last run asked the frame loop})."""
    asked = {}

    class Stub(P.Pipeline):
        def __init__(self, output_frames):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = output_frames, False, 2, {}, None, torch.device('cuda:0')

        def estimate(self, tensorImage):
            return self.objectCommon

    def kenburns(settings, oc, module, keep_on_device=False):
        asked['keep_on_device'] = keep_on_device
        return in_hbm if keep_on_device else [f for f in raw]
    monkeypatch.setattr(P.common, 'process_kenburns', kenburns)
    monkeypatch.setattr(P.shutil, 'which', lambda name: None)
    return Stub, asked
