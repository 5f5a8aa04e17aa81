"""The crop + exact area-average reduction on the GPU (include/kbe_crop_area.h; kernel: csrc/kbe_crop_area.hip): kbe_crop_area_u8 byte for
byte against the NumPy twin (tests/crop_area_cases.py) under guard bands and both poisons, padded strides, unaligned pointers and argument
checks, and the host side built on it (crop_area.reduce, common.render_frames(out_size=), Pipeline(width=))."""
import ctypes
import io
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import crop_area_cases as cc
import encoder_gpu as eg
import filter_gpu as fg

pytestmark = pytest.mark.gpu
POISONS = (0x00, 0xFF)
EVERY_CROP = [(frame, name) for frame in cc.FRAMES for name in sorted(cc.OFF)]


@pytest.fixture(scope='module')
def CA():
    from ken_burns_effect_amd import crop_area
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    crop_area.load()
    return crop_area


stream, run = fg.stream, fg.run_crop_area             # (the raw call on guarded buffers: tests/filter_gpu.py)


def assert_reduced(CA, frames, crop, size, want, poisons=POISONS, **kw):
    (w, h), n = size, len(frames)
    for poison in poisons:
        rc, got = run(CA, frames, crop, size, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * w].reshape(n, h, w, 3), want), (crop, size, poison)
        assert (got[:, :, 3 * w:] == poison).all()                       # the rows' padding is not written


@pytest.mark.parametrize('frame, name', EVERY_CROP, ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(CA, frame, name):
    """37x50, 64x48 and 160x128 frames, crops of all four parities and of the frame's own sides, to one pixel, to the patch itself, to just
    under a factor of 2 and 7-fold; 2 frames."""
    crop = cc.crop_of(frame, name)
    for size in cc.targets(crop).values():
        assert_reduced(CA, cc.frames(*frame), crop, size, cc.twin_of(frame[0], frame[1], crop, size))


@pytest.mark.parametrize('crop', [(690, 19), (689, 19), (690, 18)], ids=['eo', 'oo', 'ee'])
def test_a_crop_wider_than_a_strip_and_one_taller(CA, crop):
    """700x20, crop 690x19 (689x19: on whole pixels; 690x18: on half pixels on both axes) -> 345x7: six tiles across, the 19 rows two strips
    of 16 down; -> 64x3: ONE tile whose span is all 690 patch pixels -- three strips of 339 across, each with its extra raw pixel -- and
    all the rows.  And the transpose, 20x700: -> 3x64 a tile's 4 rows span 44 patch rows, three strips down."""
    frame = cc.wide()
    for size in ((345, 7), (64, 3)):
        assert_reduced(CA, frame, crop, size, cc.twin_reduce(frame, crop, size), poisons=(0xFF,))
    tall = np.ascontiguousarray(frame.transpose(0, 2, 1, 3))
    crop = crop[::-1]
    for size in ((7, 345), (3, 64)):
        assert_reduced(CA, tall, crop, size, cc.twin_reduce(tall, crop, size), poisons=(0xFF,))


@pytest.mark.parametrize('n', [1, 12, 13])
def test_the_launch_split(CA, n):
    """At most twelve frames a launch: 1, 12, and 13 that take two."""
    W, H = cc.FRAMES[2]
    crop = cc.crop_of((W, H), 'ee')
    assert_reduced(CA, cc.frames(W, H, n), crop, (75, 60), cc.twin_of(W, H, crop, (75, 60), n), poisons=(0xFF,))


@pytest.mark.parametrize('name', ['ee', 'oe', 'oo', 'full'])
def test_padded_strides_and_unaligned_pointers(CA, name):
    """Source rows 7 bytes apart beyond their pixels (every row at another alignment), output rows 5, the source and the output 1, 2 and 3
    bytes off their allocations: the twin's bytes, the padding of every row and the bands around every frame untouched."""
    W, H = cc.FRAMES[2]
    crop = cc.crop_of((W, H), name)
    for size in (cc.targets(crop)['under_2'], crop):
        want = cc.twin_of(W, H, crop, size)
        assert_reduced(CA, cc.frames(W, H), crop, size, want, pad=7, out_pad=5, shift=3, src_shift=1)
        assert_reduced(CA, cc.frames(W, H), crop, size, want, pad=1, out_pad=0, shift=1, src_shift=2, poisons=(0xFF,))
        assert_reduced(CA, cc.frames(W, H), crop, size, want, pad=0, out_pad=2, shift=2, src_shift=3, poisons=(0x00,))


@pytest.mark.parametrize('frame', cc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_a_crop_on_whole_pixels_is_area_reduce_on_offset_views(CA, frame):
    """W - cw and H - ch odd: kbe_area_reduce_u8 on the raw rectangle where it lies -- the frames' pointers moved to its first pixel, the rows
    still the frame's stride apart -- gives the same bytes, both on the device."""
    from ken_burns_effect_amd import area
    W, H = frame
    cw, ch = cc.crop_of(frame, 'oo')
    x, y = (W - cw + 1) // 2, (H - ch + 1) // 2
    raw = torch.from_numpy(np.array(cc.frames(W, H))).cuda()
    for w, h in cc.targets((cw, ch)).values():
        got = CA.reduce(raw, (cw, ch), (w, h))
        other = torch.full((2, h, w, 3), 0x5A, dtype=torch.uint8, device='cuda')
        views = (ctypes.c_void_p * 2)(*[raw.data_ptr() + (i * H + y) * 3 * W + 3 * x for i in range(2)])
        outs = (ctypes.c_void_p * 2)(*[other.data_ptr() + i * h * w * 3 for i in range(2)])
        assert area._raw('kbe_area_reduce_u8', views, 2, cw, ch, 3 * W, outs, w, h, 3 * w, stream()) == 0
        assert torch.equal(got, other), (w, h)


REFUSALS = {'null frames': lambda a: a.update(frames_u8=None),
            'null output 1': lambda a: a['out_u8'].__setitem__(1, None),
            'n = 0': lambda a: a.update(n_frames=0),
            'W = 65536': lambda a: a.update(W=65536, stride_bytes=3 * 65536),
            'crop_w > W': lambda a: a.update(crop_w=a['W'] + 1),
            'crop_h = 0': lambda a: a.update(crop_h=0),
            'w > crop_w': lambda a: a.update(w=a['crop_w'] + 1, out_stride_bytes=3 * (a['crop_w'] + 1)),
            'h > crop_h': lambda a: a.update(h=a['crop_h'] + 1),
            'stride < 3 W': lambda a: a.update(stride_bytes=3 * a['W'] - 1),
            'out stride < 3 w': lambda a: a.update(out_stride_bytes=3 * a['w'] - 1)}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(CA, what):
    from ken_burns_effect_amd import _native
    W, H = cc.FRAMES[0]
    rc, got = run(CA, cc.frames(W, H), (33, 44), (3, 5), change=REFUSALS[what], poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode().startswith('kbe_crop_area_u8: ')
    assert (got == 0xFF).all()


def test_crop_area_reduce_and_its_refusals(CA):
    from ken_burns_effect_amd import _native
    W, H = cc.FRAMES[2]
    frames = torch.from_numpy(np.array(cc.frames(W, H, 13))).cuda()
    crop = cc.crop_of((W, H), 'oe')
    got = CA.reduce(frames, crop, (75, 60))
    assert got.shape == (13, 60, 75, 3) and got.dtype == torch.uint8 and got.device == frames.device
    assert np.array_equal(got.cpu().numpy(), cc.twin_of(W, H, crop, (75, 60), 13))
    for bad_crop, size in (((161, 128), (75, 60)), ((160, 129), (75, 60)), ((0, 5), (1, 1)), (crop, (crop[0] + 1, 60)), (crop, (75, crop[1] + 1)), (crop, (0, 5))):
        with pytest.raises(_native.KbeError, match='crop_area.reduce'):
            CA.reduce(frames, bad_crop, size)
    with pytest.raises(_native.KbeError, match='only reduced'):
        CA.reduce(frames, crop, (crop[0] + 1, 60))
    with pytest.raises(_native.KbeError):
        CA.reduce(frames.cpu(), crop, (75, 60))


# -- the route ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    """smoke()'s scene, 128 x 96 with its default windows (crop 115 x 86: 128 - 115 odd, 96 - 86 even), and its raw frames rendered once."""
    from ken_burns_effect_amd import common, synthetic
    K = eg.kernels()
    H, W = 96, 128
    image, disp = synthetic.make_rgbd(H, W, seed=0)
    depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
    oc = {'dblFocal': synthetic.FOCAL, 'dblBaseline': synthetic.BASELINE, 'intWidth': W, 'intHeight': H, 'objectDepthrange': synthetic.depthrange_of(depth),
          'tensorRawImage': image.cuda(), 'tensorRawDisparity': disp.cuda(), 'tensorRawDepth': depth.cuda()}
    oc['tensorRawPoints'] = K.depth_to_points(oc['tensorRawDepth'], synthetic.FOCAL).view(1, 3, -1)
    ofrom, oto = synthetic.default_windows(H, W)
    settings = {'dblSteps': [0.0, 0.5, 1.0], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False}
    common._reset_inpa(oc)
    cams = common.frame_cameras(settings, oc)
    raw = common.render_frames(cams, oc, None)
    raw.setflags(write=False)
    return K, settings, oc, cams, raw


@pytest.mark.parametrize('crop', [None, (114, 85), (114, 86), (128, 96)], ids=lambda v: 'default' if v is None else '%dx%d' % v)
def test_render_frames_at_a_size_is_the_twin_of_the_raw_frames(CA, scene, crop):
    """render_frames(crop, out_size=) equals the twin applied to render_frames(crop=None), fetched and left in HBM; process_kenburns passes
    the size on."""
    from ken_burns_effect_amd import common
    K, settings, oc, cams, raw = scene
    crop = common.crop_size(settings) if crop is None else crop
    size = CA.size_for(128, 96, width=64)
    assert size == (64, 48)
    want = cc.twin_reduce(raw, crop, size)
    got = common.render_frames(cams, oc, crop, out_size=size)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    in_hbm = common.render_frames(cams, oc, crop, keep_on_device=True, out_size=size)
    assert in_hbm.is_cuda and np.array_equal(in_hbm.cpu().numpy(), want)
    if crop == common.crop_size(settings):
        frames = common.process_kenburns(settings, oc, None, out_size=size)
        assert len(frames) == 3 and all(np.array_equal(f, w) for f, w in zip(frames, want))
        assert np.array_equal(common.process_kenburns(settings, oc, None, keep_on_device=True, out_size=size).cpu().numpy(), want)
        with pytest.raises(ValueError, match='needs crop'):
            common.process_kenburns(dict(settings, boolCrop=False), oc, None, out_size=size)


@pytest.mark.parametrize('crop', [(115, 86), (114, 85), (114, 86), (115, 85), (128, 96)], ids=lambda v: '%dx%d' % v)
def test_inside_the_patchs_rectangle_the_cropped_fill_is_the_full_fill(scene, crop):
    """Deviation (7) of DESIGN.md section 2, checked: a frame whose holes are filled only inside crop_window(...) -- what the cropped route
    renders -- equals the frame filled everywhere inside the rectangle of raw pixels the patch reads."""
    from ken_burns_effect_amd import common
    K, settings, oc, cams, raw = scene
    W, H = 128, 96
    state = common._prepared_cloud(K, oc)
    (ipx, hx), (ipy, hy) = cc.start(W, crop[0]), cc.start(H, crop[1])
    x1, y1 = min(ipx + crop[0] + hx, W), min(ipy + crop[1] + hy, H)
    rect = common.crop_window(W, H, *crop)
    assert rect[0] <= ipx and rect[1] <= ipy and rect[2] >= x1 - 1 and rect[3] >= y1 - 1
    for i, (focal, shift3) in enumerate(cams):
        windowed = K.render_frame(state, shift3, focal, oc['dblBaseline'], fill_rect=rect).cpu().numpy()
        full = K.render_frame(state, shift3, focal, oc['dblBaseline']).cpu().numpy()
        assert np.array_equal(windowed[ipy:y1, ipx:x1], full[ipy:y1, ipx:x1]), i
        assert np.array_equal(windowed[ipy:y1, ipx:x1], raw[i][ipy:y1, ipx:x1]), i          # (render_frames(crop=None): the frames the route reduces)


def _first_jpeg(path):
    data = open(path, 'rb').read()
    return Image.open(io.BytesIO(data[data.index(b'\xff\xd8\xff'):]))


def _files(directory):
    return sorted(str(p.relative_to(directory)) for p in directory.rglob('*') if p.is_file())


@pytest.mark.parametrize('jpeg, png', [('native', 'native'), ('pillow', 'native'), ('device', 'native'), ('device', 'device'), ('native', 'device')])
def test_every_route_writes_the_reduced_size(CA, scene, monkeypatch, tmp_path, jpeg, png):
    """Pipeline._run without models on the scene, KBE_WIDTH=64, --write-frames --gif, on the three JPEG routes and the two PNG routes: the
    video's frames, the PNG frames and the GIF are 64 x 48, the PNG frames are the returned frames, and those are the twin's."""
    from ken_burns_effect_amd import common, pipeline as P
    K, settings, oc, cams, raw = scene

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = True, False, 3, oc, None, torch.device('cuda:0')

        def estimate(self, tensorImage):
            return self.objectCommon
    monkeypatch.setattr(P.shutil, 'which', lambda name: None)
    monkeypatch.setattr(P.common, 'build_pointcloud', lambda *a: None)
    for name in ('KBE_GIF_DITHER', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS'):
        monkeypatch.delenv(name, raising=False)
    for name, value in (('KBE_GIF', '1'), ('KBE_WIDTH', '64'), ('KBE_JPEG', jpeg), ('KBE_PNG', png)):
        monkeypatch.setenv(name, value)
    zoom = {'objectFrom': settings['objectFrom'], 'objectTo': settings['objectTo']}
    frames = Stub()(torch.zeros(1, 3, 96, 128), zoom, str(tmp_path))
    want = cc.twin_reduce(raw, common.crop_size(settings), (64, 48))
    assert len(frames) == 3 and all(np.array_equal(f, w) for f, w in zip(frames, want))
    assert _files(tmp_path) == ['3d_kbe.gif', '3d_kbe.mp4', 'frames/0.png', 'frames/1.png', 'frames/2.png']
    for i, frame in enumerate(frames):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'frames' / ('%d.png' % i))).convert('RGB')), frame[:, :, ::-1])
    assert _first_jpeg(str(tmp_path / '3d_kbe.mp4')).size == (64, 48)
    gif = Image.open(str(tmp_path / '3d_kbe.gif'))
    assert gif.size == (64, 48) and gif.n_frames == 5
    # --gif-width is taken against the reduced frames
    monkeypatch.setenv('KBE_GIF_WIDTH', '32')
    Stub()(torch.zeros(1, 3, 96, 128), zoom, str(tmp_path / 'narrow'))
    assert Image.open(str(tmp_path / 'narrow' / '3d_kbe.gif')).size == (32, 24) and Image.open(str(tmp_path / 'narrow' / 'frames' / '0.png')).size == (64, 48)
    monkeypatch.setenv('KBE_GIF_WIDTH', '65')
    with pytest.raises(ValueError, match='a GIF 65 pixels wide from frames 64 wide'):
        Stub()(torch.zeros(1, 3, 96, 128), zoom, str(tmp_path / 'refused'))
    assert not (tmp_path / 'refused').exists()


def test_the_pipeline_at_a_width(CA, tmp_path, monkeypatch):
    """One Pipeline(width=100, allow_random_weights=True) call on a 256 x 192 image with --write-frames --gif: every file decodes to 100 x 75,
    the PNG frames are the returned frames, and those are the twin's reduction of the cloud's raw frames."""
    from ken_burns_effect_amd import kbe, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG'):
        monkeypatch.delenv(name, raising=False)
    image, _ = synthetic.make_rgbd(192, 256, 12)
    zoom = kbe.windows_for(256, 192, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=3, gif=True, width=100)
        frames = pipe(image, zoom, str(tmp_path))
    assert len(frames) == 3 and all(f.shape == (75, 100, 3) and f.dtype == np.uint8 for f in frames) and np.stack(frames).std() > 1.0
    assert _files(tmp_path) == ['3d_kbe.gif', '3d_kbe.mp4', 'frames/0.png', 'frames/1.png', 'frames/2.png']
    for i, frame in enumerate(frames):
        png = Image.open(str(tmp_path / 'frames' / ('%d.png' % i)))
        assert png.size == (100, 75) and np.array_equal(np.asarray(png.convert('RGB')), frame[:, :, ::-1])
    gif = Image.open(str(tmp_path / '3d_kbe.gif'))
    assert gif.size == (100, 75) and gif.n_frames == 5
    import shutil
    if shutil.which('ffmpeg') is None:                                  # (a Motion-JPEG .mp4: its first sample decodes)
        assert _first_jpeg(str(tmp_path / '3d_kbe.mp4')).size == (100, 75)
    # the frames are the twin's reduction of the same cloud's raw frames
    from ken_burns_effect_amd import common
    settings = {'dblSteps': np.linspace(0.0, 1.0, 3).tolist(), 'objectFrom': zoom['objectFrom'], 'objectTo': zoom['objectTo'], 'boolInpaint': False, 'dolly': False}
    raw = common.render_frames(common.frame_cameras(settings, pipe.objectCommon), pipe.objectCommon, None)
    assert np.array_equal(np.stack(frames), cc.twin_reduce(raw, common.crop_size(settings), (100, 75)))
