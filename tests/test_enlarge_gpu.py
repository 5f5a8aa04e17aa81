"""The crop + exact bicubic enlargement on the GPU (include/kbe_enlarge.h; kernel: csrc/kbe_enlarge.hip): kbe_enlarge_u8 byte for byte against
the NumPy twin (tests/enlarge_cases.py) under guard bands and both poisons, padded strides, unaligned pointers, the side limits and argument
checks, on a side stream, and the host side built on it (enlarge.enlarge, common.render_frames(out_size=, enlarge=True), Pipeline(enlarge=))."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import crop_area_cases as cc
import encoder_gpu as eg
import enlarge_cases as ec
import enlarge_gpu as ng

pytestmark = pytest.mark.gpu
POISONS = (0x00, 0xFF)
ids = lambda v: v if isinstance(v, str) else '%dx%d' % v                     # noqa: E731


@pytest.fixture(scope='module')
def E():
    from ken_burns_effect_amd import enlarge
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    enlarge.load()
    return enlarge


run = ng.run_enlarge                                   # (the raw call on guarded buffers: tests/enlarge_gpu.py)


def assert_enlarged(E, frames, crop, size, want, poisons=POISONS, **kw):
    (w, h), n = size, len(frames)
    for poison in poisons:
        rc, got = run(E, frames, crop, size, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * w].reshape(n, h, w, 3), want), (crop, size, poison)
        assert (got[:, :, 3 * w:] == poison).all()                       # the rows' padding is not written


@pytest.mark.parametrize('frame, name', ec.EVERY_CROP, ids=ids)
def test_the_device_is_the_twin_byte_for_byte(E, frame, name):
    """37x50, 64x48 and 160x128 frames, crops of all four parities and of the frame's own sides, to the crop itself, one more on each axis
    alone and on both, just under a factor of 2, exactly 2 and 3 x + 1; 2 frames."""
    crop = ec.crop_of(frame, name)
    for size in ec.targets(crop).values():
        assert_enlarged(E, ec.frames(*frame), crop, size, ec.twin_of(frame[0], frame[1], crop, size))


@pytest.mark.parametrize('frame, crop', ec.SMALL, ids=ids)
def test_sevenfold(E, frame, crop):
    """A crop at most 23 pixels on a side, 7-fold: a tile's span is 10 or 11 patch pixels, and most taps of a tile are shared."""
    size = (7 * crop[0], 7 * crop[1])
    assert_enlarged(E, ec.frames(*frame), crop, size, ec.twin_of(frame[0], frame[1], crop, size))


@pytest.mark.parametrize('crop, size', [((1, 1), (5, 3)), ((2, 2), (9, 9)), ((1, 2), (1, 2)), ((1, 1), (1, 1))], ids=lambda v: '%dx%d' % v)
def test_degenerate_crops(E, crop, size):
    """1x1 -> 5x3 gives the constant; 2x2 -> 9x9 has every tap clamped; both parities of the frame's sides."""
    for frame in ((37, 50), (64, 48)):
        want = ec.twin_enlarge(ec.frames(*frame), crop, size)
        if crop == (1, 1):
            assert (want == cc.twin_patch(ec.frames(*frame), 1, 1)).all()
        assert_enlarged(E, ec.frames(*frame), crop, size, want)


@pytest.mark.parametrize('crop', [(33, 5), (32, 5), (33, 4)], ids=['oo', 'eo', 'oe'])
def test_many_tiles_across_a_few_patch_pixels(E, crop):
    """37x50, crop 33x5 -> 700x11: eleven tiles across, the 64 columns of one lie within 3 patch pixels and read their neighbours; and the
    transpose, 50x37, 5x33 -> 11x700: 44 tiles down."""
    frame = ec.frames(37, 50)
    size = (700, 11)
    assert_enlarged(E, frame, crop, size, ec.twin_enlarge(frame, crop, size), poisons=(0xFF,))
    tall = np.ascontiguousarray(frame.transpose(0, 2, 1, 3))
    assert_enlarged(E, tall, crop[::-1], size[::-1], ec.twin_enlarge(tall, crop[::-1], size[::-1]), poisons=(0x00,))


def test_a_wide_crop(E):
    """700x20, crop 690x19 -> 1381x39 and 689x19 (on whole pixels) -> 1378x38: 22 tiles across, each staging its own span of the raw rows."""
    frame = ec.wide()
    for crop, size in (((690, 19), (1381, 39)), ((689, 19), (1378, 38))):
        assert_enlarged(E, frame, crop, size, ec.twin_enlarge(frame, crop, size), poisons=(0xFF,))


@pytest.mark.parametrize('n', [1, 12, 13])
def test_the_launch_split(E, n):
    """At most twelve frames a launch: 1, 12, and 13 that take two."""
    W, H = ec.FRAMES[2]
    crop = ec.crop_of((W, H), 'ee')
    assert_enlarged(E, ec.frames(W, H, n), crop, (200, 157), ec.twin_of(W, H, crop, (200, 157), n), poisons=(0xFF,))


def test_the_side_limit(E):
    """A 16383 x 1 frame, its whole crop, to 16384 x 2: the longest side there is, 256 tiles across, every row tap clamped; one more pixel on
    either side is refused with the output untouched."""
    from ken_burns_effect_amd import _native
    frame = np.ascontiguousarray(eg.tiled(1, 16383, 7)[None])
    assert frame.shape == (1, 1, 16383, 3)
    assert_enlarged(E, frame, (16383, 1), (16384, 2), ec.twin_enlarge(frame, (16383, 1), (16384, 2)))
    for change, text in ((lambda a: a.update(w=16385, out_stride_bytes=3 * 16385), 'w outside crop_w..16384'), (lambda a: a.update(h=16385), 'h outside crop_h..16384')):
        rc, got = run(E, frame, (16383, 1), (16384, 2), change=change, poison=0xFF)
        assert rc == -1 and _native.load().kbe_last_error().decode().startswith('kbe_enlarge_u8: ' + text)
        assert (got == 0xFF).all()


@pytest.mark.parametrize('name', ['ee', 'oe', 'oo', 'full'])
def test_padded_strides_and_unaligned_pointers(E, name):
    """Source rows 7 bytes apart beyond their pixels (every row at another alignment), output rows 5, the source and the output 1, 2 and 3
    bytes off their allocations: the twin's bytes, the padding of every row and the bands around every frame untouched."""
    W, H = ec.FRAMES[2]
    crop = ec.crop_of((W, H), name)
    for size in (ec.targets(crop)['under_2'], crop):
        want = ec.twin_of(W, H, crop, size)
        assert_enlarged(E, ec.frames(W, H), crop, size, want, pad=7, out_pad=5, shift=3, src_shift=1)
        assert_enlarged(E, ec.frames(W, H), crop, size, want, pad=1, out_pad=0, shift=1, src_shift=2, poisons=(0xFF,))
        assert_enlarged(E, ec.frames(W, H), crop, size, want, pad=0, out_pad=2, shift=2, src_shift=3, poisons=(0x00,))


REFUSALS = {'null frames': lambda a: a.update(frames_u8=None),
            'null out': lambda a: a.update(out_u8=None),
            'null frame 0': lambda a: a['frames_u8'].__setitem__(0, None),
            'null output 1': lambda a: a['out_u8'].__setitem__(1, None),
            'n = 0': lambda a: a.update(n_frames=0),
            'W = 65536': lambda a: a.update(W=65536, stride_bytes=3 * 65536),
            'crop_w > W': lambda a: a.update(crop_w=a['W'] + 1),
            'crop_h > H': lambda a: a.update(crop_h=a['H'] + 1),
            'crop_h = 0': lambda a: a.update(crop_h=0),
            'w < crop_w': lambda a: a.update(w=a['crop_w'] - 1),
            'h < crop_h': lambda a: a.update(h=a['crop_h'] - 1),
            'stride < 3 W': lambda a: a.update(stride_bytes=3 * a['W'] - 1),
            'out stride < 3 w': lambda a: a.update(out_stride_bytes=3 * a['w'] - 1)}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(E, what):
    from ken_burns_effect_amd import _native
    W, H = ec.FRAMES[0]
    rc, got = run(E, ec.frames(W, H), (33, 44), (40, 50), change=REFUSALS[what], poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode().startswith('kbe_enlarge_u8: ')
    assert (got == 0xFF).all()


def test_on_a_side_stream(E):
    """As tests/test_streams_gpu.py holds the other filters: the raw call with a side stream's handle behind a delay, the right frames copied
    over the decoy only behind that delay; bit for bit what the default stream gives."""
    import stream_gpu as sg
    n, (W, H), crop, (w, h) = 3, (50, 37), (45, 33), (101, 70)
    rng = np.random.default_rng(3)
    right, decoy = (torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda() for _ in range(2))
    frames, out = decoy.clone(), torch.zeros(n, h, w, 3, dtype=torch.uint8, device='cuda')
    pointers = lambda t: (ctypes.c_void_p * len(t))(*[t[i].data_ptr() for i in range(len(t))])         # noqa: E731

    def call():
        E._call('kbe_enlarge_u8', pointers(frames), n, W, H, 3 * W, crop[0], crop[1], pointers(out), w, h, 3 * w, ng.stream())
        return out
    got, want = sg.hold('enlarge_u8', 'bits', [frames], [right], [decoy], call, written=lambda: [out])
    assert np.array_equal(want[0], ec.twin_enlarge(right.cpu().numpy(), crop, (w, h)))


def test_enlarge_enlarge_and_its_refusals(E):
    from ken_burns_effect_amd import _native
    W, H = ec.FRAMES[2]
    frames = torch.from_numpy(np.array(ec.frames(W, H, 13))).cuda()
    crop = ec.crop_of((W, H), 'oe')
    got = E.enlarge(frames, crop, (200, 157))
    assert got.shape == (13, 157, 200, 3) and got.dtype == torch.uint8 and got.device == frames.device
    assert np.array_equal(got.cpu().numpy(), ec.twin_of(W, H, crop, (200, 157), 13))
    for bad_crop, size in (((161, 128), (200, 157)), ((160, 129), (200, 157)), ((0, 5), (1, 1)), (crop, (crop[0] - 1, 157)), (crop, (200, crop[1] - 1)), (crop, (16385, 157)),
                           (crop, (200, 16385))):
        with pytest.raises(_native.KbeError, match='enlarge.enlarge'):
            E.enlarge(frames, bad_crop, size)
    with pytest.raises(_native.KbeError, match='only enlarged'):
        E.enlarge(frames, crop, (crop[0] - 1, 157))
    with pytest.raises(_native.KbeError):
        E.enlarge(frames.cpu(), crop, (200, 157))


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


def test_render_frames_enlarged_is_the_twin_of_the_raw_frames(E, scene):
    """render_frames(crop, out_size=(256, 192), enlarge=True) equals the twin applied to render_frames(crop=None), fetched and left in HBM;
    process_kenburns passes it on; an out_size within the crop is the reduction's, with or without the keyword."""
    from ken_burns_effect_amd import _native, common
    K, settings, oc, cams, raw = scene
    crop = common.crop_size(settings)
    assert crop == (115, 86)
    size = E.size_for(128, 96, 256)
    assert size == (256, 192)
    want = ec.twin_enlarge(raw, crop, size)
    got = common.render_frames(cams, oc, crop, out_size=size, enlarge=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    in_hbm = common.render_frames(cams, oc, crop, keep_on_device=True, out_size=size, enlarge=True)
    assert in_hbm.is_cuda and np.array_equal(in_hbm.cpu().numpy(), want)
    frames = common.process_kenburns(settings, oc, None, out_size=size, enlarge=True)
    assert len(frames) == 3 and all(np.array_equal(f, w) for f, w in zip(frames, want))
    assert np.array_equal(common.process_kenburns(settings, oc, None, keep_on_device=True, out_size=size, enlarge=True).cpu().numpy(), want)
    with pytest.raises(_native.KbeError, match='only reduced'):                                    # (without the keyword a size above the crop is refused, as before)
        common.render_frames(cams, oc, crop, out_size=size)
    assert np.array_equal(common.render_frames(cams, oc, crop, out_size=(64, 48), enlarge=True), cc.twin_reduce(raw, crop, (64, 48)))


def _first_jpeg(path):
    data = open(path, 'rb').read()
    return Image.open(io.BytesIO(data[data.index(b'\xff\xd8\xff'):]))


def _files(directory):
    return sorted(str(p.relative_to(directory)) for p in directory.rglob('*') if p.is_file())


def _stub(P, oc):
    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = True, False, 3, oc, None, torch.device('cuda:0')

        def estimate(self, tensorImage):
            return self.objectCommon
    return Stub()


@pytest.mark.parametrize('jpeg, png', [('native', 'native'), ('device', 'native'), ('device', 'device'), ('native', 'device')])
def test_every_route_writes_the_enlarged_size(E, scene, monkeypatch, tmp_path, jpeg, png):
    """Pipeline._run without models on the scene, KBE_WIDTH=256 KBE_ENLARGE=1, --write-frames --gif, on the JPEG and PNG routes, native and
    device: the video's frames, the PNG frames and the GIF are 256 x 192, the PNG frames are the returned frames, and those are the twin's."""
    from ken_burns_effect_amd import common, pipeline as P
    K, settings, oc, cams, raw = scene
    monkeypatch.setattr(P.shutil, 'which', lambda name: None)
    monkeypatch.setattr(P.common, 'build_pointcloud', lambda *a: None)
    for name in ('KBE_GIF_DITHER', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS'):
        monkeypatch.delenv(name, raising=False)
    for name, value in (('KBE_GIF', '1'), ('KBE_WIDTH', '256'), ('KBE_ENLARGE', '1'), ('KBE_JPEG', jpeg), ('KBE_PNG', png)):
        monkeypatch.setenv(name, value)
    zoom = {'objectFrom': settings['objectFrom'], 'objectTo': settings['objectTo']}
    frames = _stub(P, oc)(torch.zeros(1, 3, 96, 128), zoom, str(tmp_path))
    want = ec.twin_enlarge(raw, common.crop_size(settings), (256, 192))
    assert len(frames) == 3 and all(np.array_equal(f, w) for f, w in zip(frames, want))
    assert _files(tmp_path) == ['3d_kbe.gif', '3d_kbe.mp4', 'frames/0.png', 'frames/1.png', 'frames/2.png']
    for i, frame in enumerate(frames):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'frames' / ('%d.png' % i))).convert('RGB')), frame[:, :, ::-1])
    assert _first_jpeg(str(tmp_path / '3d_kbe.mp4')).size == (256, 192)
    gif = Image.open(str(tmp_path / '3d_kbe.gif'))
    assert gif.size == (256, 192) and gif.n_frames == 5
    # --gif-width stays at most the frames' width
    monkeypatch.setenv('KBE_GIF_WIDTH', '257')
    with pytest.raises(ValueError, match='a GIF 257 pixels wide from frames 256 wide'):
        _stub(P, oc)(torch.zeros(1, 3, 96, 128), zoom, str(tmp_path / 'refused'))
    assert not (tmp_path / 'refused').exists()


def test_a_width_within_the_crop_gives_the_reductions_bytes(E, scene, monkeypatch):
    """KBE_WIDTH=64 KBE_ENLARGE=1: the frames are the crop's area reduction, as without the switch."""
    from ken_burns_effect_amd import common, pipeline as P
    K, settings, oc, cams, raw = scene
    monkeypatch.setattr(P.common, 'build_pointcloud', lambda *a: None)
    for name in ('KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_JPEG', 'KBE_PNG'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('KBE_WIDTH', '64')
    monkeypatch.setenv('KBE_ENLARGE', '1')
    zoom = {'objectFrom': settings['objectFrom'], 'objectTo': settings['objectTo']}
    frames = _stub(P, oc)(torch.zeros(1, 3, 96, 128), zoom, None)
    want = cc.twin_reduce(raw, common.crop_size(settings), (64, 48))
    assert len(frames) == 3 and all(np.array_equal(f, w) for f, w in zip(frames, want))
