"""The depth-of-field blur on the GPU (include/kbe_dof.h; kernel: csrc/kbe_dof.hip): kbe_dof_u8 byte for byte against the NumPy twin
(tests/dof_cases.py) under guard bands and both poisons, at the shapes where the kernel can go wrong, with padded strides, unaligned pointers,
special depths and every refusal, and the host side built on it (dof.apply, common.render_frames(lens=), Pipeline(aperture=))."""
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import dof_cases as dc
import encoder_gpu as eg
import filter_gpu as fg
import gif_cases as gc

pytestmark = pytest.mark.gpu
POISONS = (0x00, 0xFF)


@pytest.fixture(scope='module')
def DOF():
    from ken_burns_effect_amd import dof
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    dof.load()
    return dof


stream, run = fg.stream, fg.run_dof                   # (the raw call on guarded buffers: tests/filter_gpu.py)


def assert_blurred(DOF, frames, depths, focus, A, R, want, poisons=POISONS, **kw):
    n, H, W, _ = np.shape(frames)
    for poison in poisons:
        rc, got = run(DOF, frames, depths, focus, A, R, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * W].reshape(n, H, W, 3), want), (W, H, R, poison)
        assert (got[:, :, 3 * W:] == poison).all()                       # the rows' padding is not written


@pytest.mark.parametrize('R', dc.RADII)
@pytest.mark.parametrize('frame', dc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(DOF, frame, R):
    """37x50, 64x48 and 160x128 frames at R = 0, 1, 5 and 16; two frames whose focus depths differ in one launch; output rows padded by 4."""
    W, H = frame
    assert_blurred(DOF, dc.frames(W, H), dc.depths(W, H), dc.focus_of(2), dc.APERTURE, R, dc.twin_of(W, H, R), out_pad=4)


@pytest.mark.parametrize('frame', [(5, 7), (7, 5), (129, 33)], ids=lambda v: '%dx%d' % v)
def test_frames_smaller_than_the_halo_and_one_pixel_beyond_the_tiles(DOF, frame):
    """5x7 and 7x5 at R = 16: the whole frame lies inside every pixel's window and most of the window outside the frame.  129x33: one pixel
    beyond two tiles across and beyond a tile's height twice."""
    W, H = frame
    frames, depths = dc.frames(W, H), dc.depths(W, H)
    want = dc.twin_of(W, H, 16)
    assert (want != frames).mean() > 0.3
    assert_blurred(DOF, frames, depths, dc.focus_of(2), dc.APERTURE, 16, want)


@pytest.mark.parametrize('where', ['column 64', 'column 63', 'row 16', 'corners'])
def test_a_disc_in_two_tiles_halos_and_in_the_corners(DOF, where):
    """200x40, everything in focus but one column on a tile's border (its disc of radius 16 lies in two tiles' halos), one row on one, or a
    4 x 4 block in each corner at radius 3: in front of the rest, so they spill over it."""
    W, H = 200, 40
    corners = [(x0 + x, y0 + y) for x0 in (0, W - 4) for y0 in (0, H - 4) for x in range(4) for y in range(4)]
    marks, A = {'column 64': ([(64, y) for y in range(H)], 16.0), 'column 63': ([(63, y) for y in range(H)], 16.0), 'row 16': ([(x, 16) for x in range(W)], 16.0),
                'corners': (corners, 3.0)}[where]
    frame = gc.photo_like(H, W, 21)[None]
    depth = dc.marked(W, H, marks)[None]
    r = dc.twin_radius(depth[0], 100.0, A, 16)
    assert r.max() == int(A) and (r > 0).sum() == len(marks)
    want = dc.twin_blur(frame, depth, [100.0], A, 16)
    changed = (want != frame).any(axis=(0, 3))
    assert changed.sum() > 100
    if where.startswith('column'):
        assert changed[:, 48:64].any() and changed[:, 64:80].any() and not changed[:, :47].any() and not changed[:, 81:].any()
    if where == 'corners':
        assert all(changed[y, x] for x in (0, W - 1) for y in (0, H - 1)) and changed[:8, 4:8].any() and not changed[8:H - 8].any()
    assert_blurred(DOF, frame, depth, [100.0], A, 16, want)


def test_thirteen_frames_cross_the_cut_into_launches(DOF):
    W, H = dc.FRAMES[0]
    assert_blurred(DOF, dc.frames(W, H, 13), dc.depths(W, H, 13), dc.focus_of(13), dc.APERTURE, 5, dc.twin_of(W, H, 5, 13), poisons=(0xFF,))


@pytest.mark.parametrize('frame', [dc.FRAMES[0], dc.FRAMES[2]], ids=lambda v: '%dx%d' % v)
def test_padded_strides_and_unaligned_pointers(DOF, frame):
    """Source rows 5 bytes apart beyond their pixels (every row at another alignment), depth rows 3 floats, output rows 7 bytes, the source
    and the output 1, 2 and 3 bytes off their allocations: the twin's bytes, the padding of every row and the bands around every frame untouched."""
    W, H = frame
    args = (dc.frames(W, H), dc.depths(W, H), dc.focus_of(2), dc.APERTURE, 16, dc.twin_of(W, H, 16))
    assert_blurred(DOF, *args, pad=5, z_pad=3, out_pad=7, shift=3, src_shift=1)
    assert_blurred(DOF, *args, pad=5, z_pad=0, out_pad=7, shift=1, src_shift=2, poisons=(0xFF,))
    assert_blurred(DOF, *args, pad=0, z_pad=3, out_pad=0, shift=2, src_shift=3, poisons=(0x00,))


def test_special_depths_give_radius_0_on_the_device(DOF):
    """NaN, +inf, 0 and -5 among the depths: such a pixel keeps its bytes unless a neighbour spills over it, and spills over nobody, as in the twin."""
    W, H = dc.FRAMES[1]
    depths = np.array(dc.depths(W, H))
    for k, special in enumerate((np.nan, np.inf, 0.0, -5.0)):
        depths[0, k::9, k::7] = special
        depths[1, 10 + 8 * k:14 + 8 * k, 5:60] = special
    want = dc.twin_blur(dc.frames(W, H), depths, dc.focus_of(2), dc.APERTURE, 16)
    assert (dc.twin_radius(depths, 120.0, dc.APERTURE, 16)[~(np.isfinite(depths) & (depths > 0))] == 0).all()
    assert not np.array_equal(want, dc.twin_of(W, H, 16))
    assert_blurred(DOF, dc.frames(W, H), depths, dc.focus_of(2), dc.APERTURE, 16, want)
    # a plane of nothing but specials: the frame itself
    assert_blurred(DOF, dc.frames(W, H), np.full((2, H, W), np.nan, np.float32), dc.focus_of(2), dc.APERTURE, 16, dc.frames(W, H), poisons=(0xFF,))


def _out_bytes(a):
    return (a['H'] - 1) * a['out_stride_bytes'] + 3 * a['W']


REFUSALS = {'null frames': (lambda a: a.update(frames_u8=None), 'null frames_u8'),
            'null depths': (lambda a: a.update(depth_f32=None), 'null depth_f32'),
            'null focus': (lambda a: a.update(focus=None), 'null focus'),
            'null outputs': (lambda a: a.update(out_u8=None), 'null out_u8'),
            'null frame 1': (lambda a: a['frames_u8'].__setitem__(1, None), 'null element of frames_u8'),
            'null plane 0': (lambda a: a['depth_f32'].__setitem__(0, None), 'null element of depth_f32'),
            'null output 1': (lambda a: a['out_u8'].__setitem__(1, None), 'null element of out_u8'),
            'n = 0': (lambda a: a.update(n_frames=0), 'n_frames < 1'),
            'W = 65536': (lambda a: a.update(W=65536, stride_bytes=3 * 65536, depth_stride_floats=65536, out_stride_bytes=3 * 65536), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'depth stride < W': (lambda a: a.update(depth_stride_floats=a['W'] - 1), 'depth_stride_floats < W'),
            'out stride < 3 W': (lambda a: a.update(out_stride_bytes=3 * a['W'] - 1), 'out_stride_bytes < 3 W'),
            'radius 17': (lambda a: a.update(max_radius=17), 'max_radius outside 0..16'),
            'radius -1': (lambda a: a.update(max_radius=-1), 'max_radius outside 0..16'),
            'aperture -1': (lambda a: a.update(aperture=-1.0), 'aperture is not a finite number >= 0'),
            'aperture inf': (lambda a: a.update(aperture=float('inf')), 'aperture is not a finite number >= 0'),
            'aperture nan': (lambda a: a.update(aperture=float('nan')), 'aperture is not a finite number >= 0'),
            'focus 0': (lambda a: a['focus'].__setitem__(1, 0.0), 'an element of focus is not a finite number > 0'),
            'focus -2': (lambda a: a['focus'].__setitem__(0, -2.0), 'an element of focus is not a finite number > 0'),
            'focus nan': (lambda a: a['focus'].__setitem__(1, float('nan')), 'an element of focus is not a finite number > 0'),
            'focus inf': (lambda a: a['focus'].__setitem__(0, float('inf')), 'an element of focus is not a finite number > 0'),
            'output is a source': (lambda a: a['out_u8'].__setitem__(1, a['frames_u8'][1]), 'an element of out_u8 overlaps a source frame'),
            'output is the other source': (lambda a: a['out_u8'].__setitem__(0, a['frames_u8'][1]), 'an element of out_u8 overlaps a source frame'),
            # (the frames lie a gap apart: the output ends on the first byte of the next source and touches no other)
            'one byte of the next source': (lambda a: a['out_u8'].__setitem__(0, a['frames_u8'][1] - _out_bytes(a) + 1), 'an element of out_u8 overlaps a source frame'),
            # (the last byte of plane 0, and on into plane 1)
            'one byte of a depth plane': (lambda a: a['out_u8'].__setitem__(1, a['depth_f32'][1] - 1), 'an element of out_u8 overlaps a depth plane')}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(DOF, what):
    from ken_burns_effect_amd import _native
    W, H = dc.FRAMES[0]
    change, text = REFUSALS[what]
    rc, got = run(DOF, dc.frames(W, H), dc.depths(W, H), dc.focus_of(2), dc.APERTURE, 16, gap=3 * W * H + 64, change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_dof_u8: ' + text
    assert (got == 0xFF).all()


def test_dof_apply_and_its_refusals(DOF):
    from ken_burns_effect_amd import _native
    W, H = dc.FRAMES[2]
    frames = torch.from_numpy(np.array(dc.frames(W, H, 13))).cuda()
    depths = torch.from_numpy(np.array(dc.depths(W, H, 13))).cuda()
    got = DOF.apply(frames, depths, dc.focus_of(13), dc.APERTURE, 5)
    assert got.shape == frames.shape and got.dtype == torch.uint8 and got.device == frames.device and got.data_ptr() != frames.data_ptr()
    assert np.array_equal(got.cpu().numpy(), dc.twin_of(W, H, 5, 13))
    # the depths where they lie as plane 3 of float renders [n,4,H,W]; the default cap is 16
    renders = torch.zeros(2, 4, H, W, device='cuda')
    renders[:, 3] = depths[:2]
    assert np.array_equal(DOF.apply(frames[:2], renders[:, 3], dc.focus_of(2), dc.APERTURE).cpu().numpy(), dc.twin_of(W, H, 16))
    for bad in ((frames, depths[:12], dc.focus_of(13)), (frames, depths, dc.focus_of(12)), (frames, depths.double(), dc.focus_of(13)), (frames, depths.cpu(), dc.focus_of(13)),
                (frames, depths.transpose(1, 2), dc.focus_of(13)), (frames[0], depths[0], dc.focus_of(1))):
        with pytest.raises(_native.KbeError, match='dof.apply'):
            DOF.apply(*bad, dc.APERTURE)
    with pytest.raises(_native.KbeError, match='on the GPU'):
        DOF.apply(frames.cpu(), depths.cpu(), dc.focus_of(13), dc.APERTURE)
    with pytest.raises(_native.KbeError, match='max_radius outside 0..16'):
        DOF.apply(frames, depths, dc.focus_of(13), dc.APERTURE, 17)
    with pytest.raises(_native.KbeError, match='focus is not a finite number > 0'):
        DOF.apply(frames, depths, [0.0] * 13, dc.APERTURE)


# -- the route ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    """smoke()'s scene, 128 x 96 with its default windows (the one tests/test_crop_area_gpu.py renders), every frame rendered once on its own with
    its float render: the raw frames, their depth planes, a lens that blurs them and the twin's blur of them."""
    from ken_burns_effect_amd import common, dof, synthetic
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
    state = common._prepared_cloud(K, oc)
    raw, planes = [], []
    for focal, shift3 in cams:
        rf = torch.zeros(4, H, W, device='cuda')
        raw.append(K.render_frame(state, shift3, focal, oc['dblBaseline'], render_f32=rf).cpu().numpy().copy())
        planes.append(rf[3].cpu().numpy())
    raw, planes = np.stack(raw), np.stack(planes)
    near, far = float(np.percentile(planes[np.isfinite(planes) & (planes > 0)], 20)), float(np.percentile(planes[np.isfinite(planes) & (planes > 0)], 70))
    lens = dof.Lens(near, far, 12.0, 16)
    want = dc.twin_blur(raw, planes, dof.focus_path(near, far, 3), 12.0, 16)
    assert (want != raw).mean() > 0.2                                     # (the lens does blur this scene)
    for a in (raw, want):
        a.setflags(write=False)
    return K, settings, oc, cams, raw, lens, want


def test_render_frames_with_a_lens_is_the_twin_of_the_frames_and_their_depths(DOF, scene):
    from ken_burns_effect_amd import common
    K, settings, oc, cams, raw, lens, want = scene
    before = common.render_frames(cams, oc, None)
    assert np.array_equal(before, raw)
    in_hbm = common.render_frames(cams, oc, crop=None, keep_on_device=True, lens=lens)
    assert in_hbm.is_cuda and in_hbm.dtype == torch.uint8 and np.array_equal(in_hbm.cpu().numpy(), want)
    fetched = common.render_frames(cams, oc, None, lens=lens)
    assert isinstance(fetched, np.ndarray) and np.array_equal(fetched, want)
    assert np.array_equal(common.render_frames(cams, oc, None, lens=tuple(lens)), want)                  # (a plain tuple is taken)
    # without the lens the frames are what they were: no state leaks
    assert np.array_equal(common.render_frames(cams, oc, None), before)
    crop = common.crop_size(settings)
    cropped = common.render_frames(cams, oc, crop)
    common.render_frames(cams, oc, crop, lens=lens)
    assert np.array_equal(common.render_frames(cams, oc, crop), cropped)


def test_with_a_crop_and_with_a_size_the_blurred_frames_go_on_as_raw_frames_do(DOF, scene):
    from ken_burns_effect_amd import common, crop_area
    K, settings, oc, cams, raw, lens, want = scene
    crop = common.crop_size(settings)
    blurred = torch.from_numpy(np.array(want)).cuda()
    resized = np.stack([K.crop_resize_u8(blurred[i], crop[0], crop[1]).cpu().numpy() for i in range(3)])
    assert np.array_equal(common.render_frames(cams, oc, crop, lens=lens), resized)
    assert np.array_equal(common.render_frames(cams, oc, crop, keep_on_device=True, lens=lens).cpu().numpy(), resized)
    size = crop_area.size_for(128, 96, width=64)
    reduced = crop_area.reduce(blurred, crop, size).cpu().numpy()
    got = common.render_frames(cams, oc, crop, out_size=size, lens=lens)
    assert got.shape == (3, 48, 64, 3) and np.array_equal(got, reduced)
    # process_kenburns passes the lens on
    frames = common.process_kenburns(settings, oc, None, lens=lens)
    assert len(frames) == 3 and all(np.array_equal(f, w) for f, w in zip(frames, resized))
    assert np.array_equal(common.process_kenburns(settings, oc, None, keep_on_device=True, out_size=size, lens=lens).cpu().numpy(), reduced)
    assert np.array_equal(np.stack(common.process_kenburns(dict(settings, boolCrop=False), oc, None, lens=lens)), want)


def test_a_lens_that_blurs_nothing_returns_the_unblurred_routes_bytes(DOF, scene):
    """An aperture so small that every radius is 0, an aperture of 0 and a cap of 0: the frames of the route without a lens, compared where
    they lie in HBM -- raw, cropped and resized, and reduced."""
    from ken_burns_effect_amd import common, crop_area, dof
    K, settings, oc, cams, raw, lens, want = scene
    crop, size = common.crop_size(settings), crop_area.size_for(128, 96, width=64)
    plain = {(c, s): common.render_frames(cams, oc, c, keep_on_device=True, out_size=s).clone() for c, s in ((None, None), (crop, None), (crop, size))}
    assert np.array_equal(plain[None, None].cpu().numpy(), raw)
    for still in (dof.Lens(lens.focus_from, lens.focus_to, 1e-6), dof.Lens(lens.focus_from, lens.focus_to, 0.0), dof.Lens(lens.focus_from, lens.focus_to, 12.0, 0)):
        for (c, s), frames in plain.items():
            assert torch.equal(common.render_frames(cams, oc, c, keep_on_device=True, out_size=s, lens=still), frames), (still, c, s)


def test_more_frames_than_a_group(DOF, scene):
    """14 cameras: two groups of the route, 12 and 2; the focus path runs over all 14."""
    from ken_burns_effect_amd import common, dof
    K, settings, oc, cams, raw, lens, want = scene
    many = common.frame_cameras(dict(settings, dblSteps=np.linspace(0.0, 1.0, 14).tolist()), oc)
    got = common.render_frames(many, oc, None, lens=lens)
    state = common._prepared_cloud(K, oc)
    focus = dof.focus_path(lens.focus_from, lens.focus_to, 14)
    for i in (0, 11, 12, 13):
        rf = torch.zeros(4, 96, 128, device='cuda')
        frame = K.render_frame(state, many[i][1], many[i][0], oc['dblBaseline'], render_f32=rf).cpu().numpy()
        assert np.array_equal(got[i], dc.twin_blur(frame[None], rf[3].cpu().numpy()[None], [focus[i]], lens.aperture, 16)[0]), i


def _files(directory):
    return sorted(str(p.relative_to(directory)) for p in directory.rglob('*') if p.is_file())


def test_the_pipeline_with_an_aperture_writes_the_files_it_writes_without(DOF, tmp_path, monkeypatch):
    """One Pipeline(aperture=..., allow_random_weights=True) call on a 64 x 48 image with --write-frames --gif beside one without the aperture:
    the same files, the same number of frames of the same size, and the PNG frames are the returned frames."""
    from ken_burns_effect_amd import kbe, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO'):
        monkeypatch.delenv(name, raising=False)
    image, _ = synthetic.make_rgbd(48, 64, 12)
    zoom = kbe.windows_for(64, 48, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), False)
    written = {}
    for name, lens in (('plain', {}), ('lens', dict(aperture=6.0, focus=(20, 30), focus_to=(50, 10)))):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=3, gif=True, **lens)
            frames = pipe(image, zoom, str(tmp_path / name))
        assert len(frames) == 3 and all(f.shape == (48, 64, 3) and f.dtype == np.uint8 for f in frames)
        assert _files(tmp_path / name) == ['3d_kbe.gif', '3d_kbe.mp4', 'frames/0.png', 'frames/1.png', 'frames/2.png']
        for i, frame in enumerate(frames):
            png = Image.open(str(tmp_path / name / 'frames' / ('%d.png' % i)))
            assert png.size == (64, 48) and np.array_equal(np.asarray(png.convert('RGB')), frame[:, :, ::-1])
        gif = Image.open(str(tmp_path / name / '3d_kbe.gif'))
        assert gif.size == (64, 48) and gif.n_frames == 5
        written[name] = np.stack(frames)
    assert written['plain'].shape == written['lens'].shape
