"""The device-side PNG encoder on the GPU (kbe_png_encode, include/kbe.h; kernels: csrc/kbe_png.hip), through ctypes: its files against
the CPU twin (tests/png_check.cpp: the same csrc/kbe_png_block.h compiled by g++) BYTE FOR BYTE -- the twin itself is held against zlib
and Pillow in tests/test_png_stream.py --, the overflow contract, the argument checks, and the host side built on it."""
import ctypes
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as pc

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 4096


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def run(K, frames, flags, cap, W=None, stride=None, n=None, status_before=7, shift=0):
    """kbe_png_encode on a uint8 device tensor [n,H,Wt,3] (W <= Wt: the rows' stride is Wt's) with a buffer of `cap` bytes (`shift` bytes off
    its allocation's start) followed by GUARD bytes, everything the call may write filled with sentinels first.
    -> (rc, offsets, status, the buffer with its guard)."""
    lib = K.lib
    count, H, Wt, _ = frames.shape
    W = Wt if W is None else W
    n = count if n is None else n
    step = H * Wt * 3
    pointers = (ctypes.c_void_p * max(n, 1))(*[frames.data_ptr() + i * step for i in range(n)])
    scratch = torch.empty((int(lib.kbe_png_scratch_bytes(W, H, max(n, 1))) + 7) // 8 + 1, dtype=torch.int64, device='cuda')
    files = torch.full((shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    offsets = torch.full((max(n, 1) + 1,), -1, dtype=torch.int64, device='cuda')
    status = torch.full((1,), status_before, dtype=torch.int32, device='cuda')
    rc = lib.kbe_png_encode(pointers, n, W, H, 3 * Wt if stride is None else stride, flags, ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(files.data_ptr() + shift),
                            ctypes.c_size_t(cap), ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = files.cpu().numpy()
    assert (got[:shift] == SENTINEL).all()
    return rc, offsets.cpu().tolist(), int(status.item()), got[shift:]


def assert_files(K, frames, flags, want, room=333, **kw):
    """The device's files of `frames` are `want`, back to back; no byte behind them is touched."""
    total = sum(len(s) for s in want)
    dev = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    rc, offsets, status, buf = run(K, dev, flags, total + room, **kw)
    assert rc == 0 and status == 0
    assert offsets == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    assert buf[:total].tobytes() == b''.join(want)
    assert (buf[total:] == SENTINEL).all()


@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_device_files_are_the_twins_byte_for_byte(K, name):
    """Every case of the CPU suite, 1, 3 and 13 frames of different content (13: two launches, the offsets carry on), RGB and BGR."""
    frames = pc.case_frames(name, 13)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    for flags in (0, pc.BGR):
        want = pc.case_twin(name, 13, flags)[0]
        for n in (1, 3, 13):
            assert_files(K, dev[:n], flags, want[:n])


def test_rows_with_a_stride_and_an_unaligned_file_buffer(K):
    frames = pc.case_frames('size_50x37', 3)
    want = pc.case_twin('size_50x37', 3)[0]
    wide = np.full((3, 50, 45, 3), 99, np.uint8)
    wide[:, :, :37] = frames
    assert_files(K, wide, 0, want, room=0, W=37)
    # the files' buffer 1, 2 and 3 bytes off a 4-byte boundary: the stores of four bytes at a time start later
    for shift in (1, 2, 3):
        assert_files(K, frames, 0, want, room=0, shift=shift)
    # ... with a segment that leaves stored and coded ones of more than one store per lane
    for name in ('noise', 'photo_like'):
        assert_files(K, pc.case_frames(name, 3), pc.BGR, pc.case_twin(name, 3, pc.BGR)[0], room=0, shift=3)


def tiled(h, w, seed):
    tile = pc.photo_like(256, 256, seed)
    return np.tile(tile, (-(-h // 256), -(-w // 256), 1))[:h, :w]


def test_the_scan_over_many_segments(K):
    """More segments than one workgroup of the scan takes (256) in one frame; the scan itself is the one kbe_mjpeg_encode uses
    (csrc/kbe_units_scan.h), whose second level tests/test_mjpeg_gpu.py reaches."""
    frames = tiled(1200, 1200, 11)[None]
    want, _, segment, _ = pc.twin(frames)
    assert -(-1200 * 3601 // segment) > 256
    assert_files(K, frames, 0, want)


def test_a_buffer_too_small_reports_the_true_sizes_and_nothing_is_written_beyond_it(K):
    frames = pc.case_frames('photo_like', 3)
    want = pc.case_twin('photo_like', 3)[0]
    joined = b''.join(want)
    sizes = np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    for cap in (len(joined) - 1, len(joined) - 2, sizes[1] + 5, 7, 0):          # one byte short; ...; inside the second and the first header; nothing
        rc, offsets, status, buf = run(K, dev, 0, cap)
        assert rc == 0 and status == 1, cap
        assert offsets == sizes, cap
        assert buf[:cap].tobytes() == joined[:cap], cap                     # (what fits is the files' beginning)
        assert (buf[cap:] == SENTINEL).all(), cap
    rc, offsets, status, buf = run(K, dev, 0, len(joined))                  # exactly enough
    assert rc == 0 and status == 0 and buf[:len(joined)].tobytes() == joined and (buf[len(joined):] == SENTINEL).all()
    # the bound is the twin's, and noise reaches it
    noisy = pc.case_twin('noise', 3)
    assert int(K.lib.kbe_png_bound(80, 100)) == noisy[3] == len(noisy[0][0])


def test_invalid_arguments_are_refused_before_anything_is_enqueued(K):
    frames = torch.from_numpy(np.ascontiguousarray(pc.case_frames('size_17x16', 3))).cuda()
    lib = K.lib

    def refused(**kw):
        rc, offsets, status, buf = run(K, frames, kw.pop('flags', 0), 4096, **kw)
        return rc == -1 and status == 7 and set(offsets) == {-1} and bool((buf == SENTINEL).all())      # KBE_E_INVALID, and nothing ran
    assert refused(n=0) and refused(n=-3)
    assert refused(flags=2) and refused(flags=-1)
    assert refused(stride=3 * 16 - 1) and refused(W=0) and refused(W=17)                                    # (W = 17 > the rows' 16 pixels: stride < 3 W)
    scratch = torch.empty(4096, dtype=torch.int64, device='cuda')
    meta = torch.full((8,), -1, dtype=torch.int64, device='cuda')
    files = torch.full((4096,), SENTINEL, dtype=torch.uint8, device='cuda')
    good = dict(frames=(ctypes.c_void_p * 3)(*[frames.data_ptr() + i * 17 * 16 * 3 for i in range(3)]), n=3, W=16, H=17, stride=48, flags=0,
                scratch=scratch.data_ptr(), files=files.data_ptr(), cap=4096, offsets=meta.data_ptr(), status=meta.data_ptr() + 56)

    def call(**change):
        a = dict(good, **change)
        return lib.kbe_png_encode(a['frames'], a['n'], a['W'], a['H'], a['stride'], a['flags'], ctypes.c_void_p(a['scratch']), ctypes.c_void_p(a['files']),
                                  ctypes.c_size_t(a['cap']), ctypes.c_void_p(a['offsets']), ctypes.c_void_p(a['status']), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(frames=None) == -1 and call(scratch=0) == -1 and call(files=0) == -1 and call(offsets=0) == -1 and call(status=0) == -1
    assert call(frames=(ctypes.c_void_p * 3)(frames.data_ptr(), None, frames.data_ptr())) == -1                # a null frame among them
    assert call(W=65536, stride=3 * 65536) == -1 and call(H=65536) == -1 and call(H=0) == -1
    assert call(W=65535, H=65535, stride=3 * 65535) == -1                                                   # a file of 2^31 bytes or more
    assert call(scratch=scratch.data_ptr() + 4) == -1 and call(offsets=meta.data_ptr() + 4) == -1            # 8-byte alignment
    torch.cuda.synchronize()
    assert bool((meta == -1).all()) and bool((files == SENTINEL).all())
    assert b'kbe_png_encode' in lib.kbe_last_error()
    assert call() == 0                                                                                      # ... and the good call goes through
    assert int(lib.kbe_png_bound(0, 5)) == 0 and int(lib.kbe_png_bound(65535, 65535)) == 0 and int(lib.kbe_png_scratch_bytes(16, 17, 0)) == 0
    assert 0 < int(lib.kbe_png_bound(30000, 23000)) < 2 ** 31 and int(lib.kbe_png_bound(30000, 24000)) == 0
    assert int(lib.kbe_png_scratch_bytes(1024, 1024, 75)) == int(lib.kbe_png_scratch_bytes(1024, 1024, 12)) < (1 << 20)        # no worst-case file in it


def test_the_tensor_level_call_and_its_second_run_with_a_larger_buffer(K):
    frames = pc.case_frames('noise', 3)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    want = pc.case_twin('noise', 3)[0]
    assert K.png_encode(dev) == want
    assert K.png_encode(dev, cap=10) == want                                # the second run with the size the first reported
    assert K.png_encode(dev, bgr=True) == pc.case_twin('noise', 3, pc.BGR)[0]
    assert K.png_encode(dev[:1], cap=1 << 20) == want[:1]
    for data, frame in zip(K.png_encode(dev), frames):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), frame)
    from ken_burns_effect_amd._native import KbeError
    with pytest.raises(KbeError):
        K.png_encode(dev.cpu())


@pytest.fixture(scope='module')
def rendered(K):
    """smoke()'s scene: two cameras, the frames left in HBM (as in tests/test_mjpeg_gpu.py)."""
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


@pytest.mark.parametrize('pretrained_estim', [False, True], ids=['bgr', 'rgb'])
@pytest.mark.parametrize('jpeg', ['native', 'device'])
def test_the_pipeline_writes_its_png_frames_from_hbm_under_the_switch(K, rendered, pretrained_estim, jpeg, monkeypatch, tmp_path):
    """Pipeline._run with KBE_PNG=device and PNG frames asked for: the frame loop is asked to leave its frames on the device, each is
    encoded once, frames/%d.png decode to the frames in RGB, the video is still written, and the frames come back as numpy arrays."""
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
    monkeypatch.setenv('KBE_PNG', 'device')
    monkeypatch.setenv('KBE_JPEG', jpeg)
    image = torch.zeros(1, 3, 96, 128)
    out = Stub(True)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is True
    assert len(out) == 2 and all(isinstance(f, np.ndarray) and np.array_equal(f, r) for f, r in zip(out, raw))
    want = pc.twin(raw, 0 if pretrained_estim else pc.BGR)[0]
    for i in range(2):
        data = open(str(tmp_path / 'frames' / ('%d.png' % i)), 'rb').read()
        assert data == want[i]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), raw[i] if pretrained_estim else raw[i][:, :, ::-1])
    assert not (tmp_path / 'frames' / '2.png').exists()
    video = open(str(tmp_path / '3d_kbe.mp4'), 'rb').read()
    assert video.count(b'\xff\xd8\xff\xe0') == 3                            # forth and back: three Motion-JPEG frames
    # no PNG frames asked for: the switch changes nothing
    monkeypatch.setenv('KBE_JPEG', 'native')
    Stub(False)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path / 'plain'), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is False and not (tmp_path / 'plain' / 'frames').exists()
    # without the switch: today's host route, today's files
    monkeypatch.delenv('KBE_PNG')
    Stub(True)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path / 'host'), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is False
    rgb = raw[1] if pretrained_estim else raw[1][:, :, ::-1]
    assert open(str(tmp_path / 'host' / 'frames' / '1.png'), 'rb').read() == P.png_bytes(rgb)


def test_one_idat_that_zlib_inflates_to_the_filtered_bytes(K):
    frame = pc.case_frames('size_17x16', 1)
    data = K.png_encode(torch.from_numpy(np.ascontiguousarray(frame)).cuda())[0]
    idat = [body for tag, body in pc.chunks(data) if tag == b'IDAT']
    assert len(idat) == 1 and zlib.decompress(idat[0]) == pc.filtered(frame[0])
