"""The device-side Motion-JPEG encoder on the GPU (kbe_mjpeg_encode, include/kbe.h; kernels: csrc/kbe_mjpeg.hip), through ctypes: its
streams against the CPU twin (tests/mjpeg_check.cpp: the same csrc/kbe_mjpeg_block.h compiled by g++) BYTE FOR BYTE -- the twin itself is
held against Pillow in tests/test_mjpeg_stream.py --, the overflow contract, the argument checks, and the host side built on it."""
import ctypes

import numpy as np
import pytest
import torch

import mjpeg_cases as mc
from test_jpeg_writer import decode, pillow, psnr

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 4096


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def run(K, frames, quality, flags, cap, W=None, stride=None, n=None, status_before=7):
    """kbe_mjpeg_encode on a uint8 device tensor [n,H,Wt,3] (W <= Wt: the rows' stride is Wt's) with a stream buffer of `cap` bytes followed
    by GUARD bytes, everything the call may write filled with sentinels first.  -> (rc, offsets, status, the buffer with its guard)."""
    lib = K.lib
    count, H, Wt, _ = frames.shape
    W = Wt if W is None else W
    n = count if n is None else n
    step = H * Wt * 3
    pointers = (ctypes.c_void_p * max(n, 1))(*[frames.data_ptr() + i * step for i in range(n)])
    scratch = torch.empty((int(lib.kbe_mjpeg_scratch_bytes(W, H, max(n, 1))) + 7) // 8 + 1, dtype=torch.int64, device='cuda')
    streams = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    offsets = torch.full((max(n, 1) + 1,), -1, dtype=torch.int64, device='cuda')
    status = torch.full((1,), status_before, dtype=torch.int32, device='cuda')
    rc = lib.kbe_mjpeg_encode(pointers, n, W, H, 3 * Wt if stride is None else stride, quality, flags, ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(streams.data_ptr()),
                              ctypes.c_size_t(cap), ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, offsets.cpu().tolist(), int(status.item()), streams.cpu().numpy()


def assert_streams(K, frames, quality, flags, want, room=333):
    """The device's streams of `frames` are `want`, back to back; no byte behind them is touched."""
    total = sum(len(s) for s in want)
    rc, offsets, status, buf = run(K, torch.from_numpy(np.ascontiguousarray(frames)).cuda(), quality, flags, total + room)
    assert rc == 0 and status == 0
    assert offsets == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    assert buf[:total].tobytes() == b''.join(want)
    assert (buf[total:] == SENTINEL).all()


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_device_streams_are_the_twins_byte_for_byte(K, name):
    """Every case of the CPU suite, 1, 3 and 13 frames of different content (13: two launches, the offsets carry on), RGB and BGR."""
    quality = mc.CASES[name][2]
    frames = mc.case_frames(name, 13)
    for flags in (0, mc.BGR):
        want = mc.case_twin(name, 13, flags)[0]
        for n in (1, 3, 13):
            assert_streams(K, frames[:n], quality, flags, want[:n])


def test_rows_with_a_stride_and_an_unaligned_stream_buffer(K):
    frames = mc.case_frames('size_50x37', 3)
    want = mc.case_twin('size_50x37', 3)[0]
    wide = np.full((3, 50, 45, 3), 99, np.uint8)
    wide[:, :, :37] = frames
    total = sum(len(s) for s in want)
    rc, offsets, status, buf = run(K, torch.from_numpy(wide).cuda(), 92, 0, total, W=37)
    assert rc == 0 and status == 0 and buf[:total].tobytes() == b''.join(want) and (buf[total:] == SENTINEL).all()
    # the streams' buffer one byte off a 4-byte boundary: the stores of four bytes at a time start later
    lib = K.lib
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    streams = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    scratch = torch.empty(int(lib.kbe_mjpeg_scratch_bytes(37, 50, 3)) // 8 + 1, dtype=torch.int64, device='cuda')
    meta = torch.zeros(5, dtype=torch.int64, device='cuda')
    pointers = (ctypes.c_void_p * 3)(*[dev.data_ptr() + i * 50 * 37 * 3 for i in range(3)])
    for shift in (1, 2, 3):
        streams.fill_(SENTINEL)
        assert lib.kbe_mjpeg_encode(pointers, 3, 37, 50, 3 * 37, 92, 0, ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(streams.data_ptr() + shift), ctypes.c_size_t(total),
                                    ctypes.c_void_p(meta.data_ptr()), ctypes.c_void_p(meta.data_ptr() + 32), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        got = streams.cpu().numpy()
        assert got[shift:shift + total].tobytes() == b''.join(want) and (got[:shift] == SENTINEL).all() and (got[shift + total:] == SENTINEL).all()


def tiled(h, w, seed):
    tile = mc.photo_like(256, 256, seed)
    return np.tile(tile, (-(-h // 256), -(-w // 256), 1))[:h, :w]


@pytest.mark.parametrize('shape', [(3, 512, 768), (1, 4096, 4112)], ids=['1152_intervals', '16448_intervals'])
def test_the_scan_over_many_intervals(K, shape):
    """More intervals than one workgroup of the scan takes (256), and more sums of 256 than the scan of the sums takes at once (64)."""
    n, h, w = shape
    frames = np.stack([tiled(h, w, 11 + i) for i in range(n)])
    want, _, R, _ = mc.twin(frames, 75)
    assert n * -(-(-(-h // 16) * -(-w // 16)) // R) > (256 if n == 3 else 64 * 256)
    assert_streams(K, frames, 75, 0, want)


def test_a_buffer_too_small_reports_the_true_sizes_and_nothing_is_written_beyond_it(K):
    frames = mc.case_frames('noise', 3)
    want = mc.case_twin('noise', 3)[0]
    joined = b''.join(want)
    sizes = np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    for cap in (len(joined) - 1, len(joined) - 2, sizes[1] + 5, 7, 0):          # one byte short; ...; inside the first header; nothing
        rc, offsets, status, buf = run(K, dev, 100, 0, cap)
        assert rc == 0 and status == 1, cap
        assert offsets == sizes, cap
        assert buf[:cap].tobytes() == joined[:cap], cap                     # (what fits is the stream's beginning)
        assert (buf[cap:] == SENTINEL).all(), cap
    rc, offsets, status, buf = run(K, dev, 100, 0, len(joined))             # exactly enough
    assert rc == 0 and status == 0 and buf[:len(joined)].tobytes() == joined and (buf[len(joined):] == SENTINEL).all()
    assert len(joined) <= 3 * int(K.lib.kbe_mjpeg_bound(80, 64)) and int(K.lib.kbe_mjpeg_bound(80, 64)) == mc.case_twin('noise', 3)[3]


def test_invalid_arguments_are_refused_before_anything_is_enqueued(K):
    frames = torch.from_numpy(np.ascontiguousarray(mc.case_frames('size_17x16', 3))).cuda()
    lib = K.lib

    def refused(**kw):
        rc, offsets, status, buf = run(K, frames, kw.pop('quality', 92), kw.pop('flags', 0), 4096, **kw)
        return rc == -1 and status == 7 and set(offsets) == {-1} and bool((buf == SENTINEL).all())      # KBE_E_INVALID, and nothing ran
    assert refused(n=0) and refused(n=-3)
    assert refused(quality=0) and refused(quality=101)
    assert refused(flags=2) and refused(flags=-1)
    assert refused(stride=3 * 16 - 1) and refused(W=0) and refused(W=17)                                    # (W = 17 > the rows' 16 pixels: stride < 3 W)
    scratch = torch.empty(4096, dtype=torch.int64, device='cuda')
    meta = torch.full((8,), -1, dtype=torch.int64, device='cuda')
    streams = torch.full((4096,), SENTINEL, dtype=torch.uint8, device='cuda')
    good = dict(frames=(ctypes.c_void_p * 3)(*[frames.data_ptr() + i * 17 * 16 * 3 for i in range(3)]), n=3, W=16, H=17, stride=48, quality=92, flags=0,
                scratch=scratch.data_ptr(), streams=streams.data_ptr(), cap=4096, offsets=meta.data_ptr(), status=meta.data_ptr() + 56)

    def call(**change):
        a = dict(good, **change)
        return lib.kbe_mjpeg_encode(a['frames'], a['n'], a['W'], a['H'], a['stride'], a['quality'], a['flags'], ctypes.c_void_p(a['scratch']), ctypes.c_void_p(a['streams']),
                                    ctypes.c_size_t(a['cap']), ctypes.c_void_p(a['offsets']), ctypes.c_void_p(a['status']), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(frames=None) == -1 and call(scratch=0) == -1 and call(streams=0) == -1 and call(offsets=0) == -1 and call(status=0) == -1
    assert call(frames=(ctypes.c_void_p * 3)(frames.data_ptr(), None, frames.data_ptr())) == -1                # a null frame among them
    assert call(W=65536, stride=3 * 65536) == -1 and call(H=65536) == -1 and call(H=0) == -1
    assert call(scratch=scratch.data_ptr() + 4) == -1 and call(offsets=meta.data_ptr() + 4) == -1            # 8-byte alignment
    torch.cuda.synchronize()
    assert bool((meta == -1).all()) and bool((streams == SENTINEL).all())
    assert b'kbe_mjpeg_encode' in lib.kbe_last_error()
    assert call() == 0                                                                                      # ... and the good call goes through
    assert int(lib.kbe_mjpeg_bound(0, 5)) == 0 and int(lib.kbe_mjpeg_scratch_bytes(16, 17, 0)) == 0
    assert int(lib.kbe_mjpeg_scratch_bytes(1024, 1024, 75)) == int(lib.kbe_mjpeg_scratch_bytes(1024, 1024, 12)) < (1 << 20)      # no worst-case stream in it


def test_the_tensor_level_call_and_its_second_run_with_a_larger_buffer(K):
    frames = mc.case_frames('noise', 3)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    want = mc.case_twin('noise', 3)[0]
    assert K.mjpeg_encode(dev, 100) == want                                 # (noise at quality 100 does not fit the first guess of a quarter of the pixels)
    assert K.mjpeg_encode(dev, 100, cap=10) == want
    assert K.mjpeg_encode(dev, 100, bgr=True) == mc.case_twin('noise', 3, mc.BGR)[0]
    assert K.mjpeg_encode(dev[:1], 100, cap=1 << 20) == want[:1]
    from ken_burns_effect_amd._native import KbeError
    with pytest.raises(KbeError):
        K.mjpeg_encode(dev.cpu(), 92)


@pytest.fixture(scope='module')
def rendered(K):
    """smoke()'s scene: two cameras, the frames left in HBM."""
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


def test_rendered_frames_encoded_where_they_lie_decode_to_the_frames_delivered_raw(K, rendered):
    in_hbm, raw = rendered
    assert in_hbm.is_cuda and raw.shape == (2, 96, 128, 3)
    streams = K.mjpeg_encode(in_hbm, 92)
    assert streams == mc.twin(raw, 92)[0]
    for stream, frame in zip(streams, raw):
        got = decode(stream)
        ours, theirs = psnr(got, frame), psnr(decode(pillow(frame, 92)), frame)
        print('device %.2f dB, Pillow %.2f dB' % (ours, theirs))
        assert got.shape == frame.shape and ours > theirs - 0.5


def test_write_video_under_the_switch_holds_the_device_streams(K, rendered, monkeypatch, tmp_path):
    from ken_burns_effect_amd import pipeline
    _, raw = rendered
    monkeypatch.setenv('KBE_JPEG', 'device')
    monkeypatch.setattr(pipeline.shutil, 'which', lambda name: None)
    assert pipeline.jpeg_encoder()[0] == 'device'
    frames = [raw[0], raw[1]]
    assert pipeline.write_video(str(tmp_path / 'v.mp4'), frames + frames[-2::-1], fps=25) is False
    want = mc.twin(raw, 92)[0]
    data = open(str(tmp_path / 'v.mp4'), 'rb').read()
    assert want[0] + want[1] + want[0] in data and data.count(b'\xff\xd8\xff\xe0') == 3
    monkeypatch.delenv('KBE_JPEG')
    assert pipeline.jpeg_encoder()[0] == 'native'                           # the default stays


@pytest.mark.parametrize('pretrained_estim', [False, True], ids=['bgr', 'rgb'])
def test_the_pipeline_keeps_its_frames_in_hbm_under_the_switch(K, rendered, pretrained_estim, monkeypatch, tmp_path):
    """Pipeline._run with KBE_JPEG=device, no ffmpeg and no PNG frames: the frame loop is asked to leave its frames on the device, each is
    encoded once (in the input's channel order), the video goes forth and back, and the frames come back as numpy arrays all the same."""
    from ken_burns_effect_amd import pipeline as P
    in_hbm, raw = rendered
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
    monkeypatch.setenv('KBE_JPEG', 'device')
    image = torch.zeros(1, 3, 96, 128)
    out = Stub(False)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is True
    assert len(out) == 2 and all(isinstance(f, np.ndarray) and np.array_equal(f, r) for f, r in zip(out, raw))
    want = mc.twin(raw, 92, 0 if pretrained_estim else mc.BGR)[0]
    data = open(str(tmp_path / '3d_kbe.mp4'), 'rb').read()
    assert want[0] + want[1] + want[0] in data
    # PNG frames asked for: today's route, whatever the switch says
    Stub(True)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path / 'png'), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is False and (tmp_path / 'png' / 'frames' / '1.png').exists()
