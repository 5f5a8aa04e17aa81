"""The shutter mean on the GPU (include/kbe_shutter.h; kernel: csrc/kbe_shutter.hip): kbe_shutter_mean_u8 byte for byte against the NumPy twin
(tests/shutter_cases.py) under guard bands and both poisons, at the shapes where the kernel can go wrong -- rows shorter than a piece, rows
around a workgroup's span, every pair of alignment classes, the cut into launches --, every refusal, a side stream, and the host side built
on it (shutter.mean, common.render_frames(shutter=), Pipeline(shutter=))."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import encoder_gpu as eg
import gif_cases as gc
import shutter_cases as sc
import shutter_gpu as sg
import stream_gpu

pytestmark = pytest.mark.gpu
run, assert_mean = sg.run_shutter, sg.assert_mean


@pytest.fixture(scope='module')
def SH():
    from ken_burns_effect_amd import shutter
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    shutter.load()
    return shutter


def assert_telling(samples, want):
    """The mean differs from every one of its samples in more than half of the bytes: a kernel that copies one sample cannot pass."""
    assert sc.differing_share(np.asarray(samples), want) > 0.5


# -- the entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize('S', sc.SAMPLES)
@pytest.mark.parametrize('frame', sc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(SH, frame, S):
    """37x50, 64x48 and 160x128 frames at S = 1, 2, 3, 8, 31 and 32; two outputs in one call; output rows padded by 4."""
    W, H = frame
    samples, want = sc.samples_of(W, H, S), sc.twin_of(W, H, S)
    if S > 1:
        assert_telling(samples, want)
    assert_mean(SH, samples, want, out_pad=4)


def _pan(W, H, S, n=1, seed=21):
    return np.stack([np.stack([gc.photo_like(H, W + S, seed + i)[:, k:k + W] for k in range(S)]) for i in range(n)])


@pytest.mark.parametrize('frame', [(1, 7), (2, 7), (5, 7), (16, 7), (1366, 3)], ids=lambda v: '%dx%d' % v)
def test_narrow_and_awkward_rows(SH, frame):
    """W = 1, 2 and 5: a row shorter than one 16-byte piece, which an unaligned row still cuts in two.  W = 16: exactly three pieces.
    1366 x 3: rows of 4098 bytes, two bytes beyond four spans.  Aligned and 13 bytes off, source rows 3 bytes apart."""
    W, H = frame
    samples = _pan(W, H, 3, n=2)
    assert_mean(SH, samples)
    assert_mean(SH, samples, pad=3, out_pad=1, shift=13, src_shift=7)


@pytest.mark.parametrize('end', [sg.SPAN - 1, sg.SPAN, sg.SPAN + 1])
def test_rows_around_a_workgroups_span(SH, end):
    """A workgroup takes SPAN = 1024 bytes of a row, counted from the row's address rounded down to 16.  Rows of 341 pixels, 1023 bytes, at an
    output stride of 1024: moved 0, 1 and 2 bytes off the allocation every row ends one byte short of the span, exactly on it, and one byte
    beyond it, in a second workgroup whose only piece is one byte.  5 rows: a second workgroup down the frame as well."""
    W, H = 341, 5
    assert sg.SPAN == 1024 and 3 * W == sg.SPAN - 1
    samples = _pan(W, H, 2)
    want = sc.twin_mean(samples)
    assert_telling(samples, want)
    assert_mean(SH, samples, want, out_pad=1, shift=end - 3 * W, aligned=True)


@pytest.mark.parametrize('shift', range(16))
def test_every_pair_of_alignment_classes(SH, shift):
    """37 x 17 frames, source rows at a stride of 117 and output rows at one of 113, so that a frame's rows walk through all sixteen classes
    modulo 16; the output moved `shift` bytes off its allocation: the sixteen calls reach all 256 pairs of (source class, output class).  The
    S = 3 samples lie an odd number of bytes apart: each has a class of its own in every row."""
    W, H, S = 37, 17, 3
    pairs = {((117 * y) % 16, (s + 113 * y) % 16) for s in range(16) for y in range(H)}
    assert len(pairs) == 256 and (H * 117) % 2 == 1 and len({(k * H * 117) % 16 for k in range(S)}) == S
    samples = _pan(W, H, S)
    want = sc.twin_mean(samples)
    assert_telling(samples, want)
    assert_mean(SH, samples, want, pad=6, out_pad=2, shift=shift, aligned=True)


def test_the_extremes(SH):
    """All-255 frames at S = 32 (every 16-bit lane at its largest), all-0 frames, and two samples (0, 1) everywhere -> 1."""
    W, H = 37, 9
    assert_mean(SH, np.full((1, 32, H, W, 3), 255, np.uint8), np.full((1, H, W, 3), 255, np.uint8))
    assert_mean(SH, np.zeros((2, 32, H, W, 3), np.uint8), np.zeros((2, H, W, 3), np.uint8))
    zero_one = np.zeros((1, 2, H, W, 3), np.uint8)
    zero_one[:, 1] = 1
    assert_mean(SH, zero_one, np.ones((1, H, W, 3), np.uint8))


def test_repeated_pointers(SH):
    """S = 4 as (a, b, b, a), and a second output as (b, b, b, a): the twin of those four."""
    W, H = 37, 20
    a, b = gc.photo_like(H, W, 3), gc.photo_like(H, W, 40)
    frames, table = np.stack([a, b]), [0, 1, 1, 0, 1, 1, 1, 0]
    want = sc.twin_mean(frames[table].reshape(2, 4, H, W, 3))
    assert (want[0] != a).mean() > 0.5 and (want[0] != b).mean() > 0.5 and not np.array_equal(want[0], want[1])
    for poison in sg.POISONS:
        rc, got = run(SH, frames, 4, table=table, poison=poison, pad=1)
        assert rc == 0 and np.array_equal(got.reshape(2, H, W, 3), want)


@pytest.mark.parametrize('n,S', [(13, 8), (4, 32), (13, 1)], ids=lambda v: str(v))
def test_the_cut_into_launches(SH, n, S):
    """A launch carries min(12, max(1, 96 / S)) outputs: 13 outputs at S = 8 are 12 + 1, 4 at S = 32 are 3 + 1, 13 at S = 1 are 12 + 1."""
    W, H = 21, 6
    samples = _pan(W, H, S, n=n)
    want = sc.twin_mean(samples)
    assert len({want[i].tobytes() for i in range(n)}) == n                  # every output is another: one taken for another shows
    assert_mean(SH, samples, want)


def _out_bytes(a):
    return (a['H'] - 1) * a['out_stride_bytes'] + 3 * a['W']


REFUSALS = {'null frames': (lambda a: a.update(frames_u8=None), 'null frames_u8'),
            'null outputs': (lambda a: a.update(out_u8=None), 'null out_u8'),
            'n = 0': (lambda a: a.update(n_out=0), 'n_out < 1'),
            'samples 0': (lambda a: a.update(samples=0), 'samples outside 1..32'),
            'samples 33': (lambda a: a.update(samples=33), 'samples outside 1..32'),
            'W = 65536': (lambda a: a.update(W=65536, stride_bytes=3 * 65536, out_stride_bytes=3 * 65536), 'W or H outside 1..65535'),
            'H = 0': (lambda a: a.update(H=0), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'out stride < 3 W': (lambda a: a.update(out_stride_bytes=3 * a['W'] - 1), 'out_stride_bytes < 3 W'),
            'null frame 3': (lambda a: a['frames_u8'].__setitem__(3, None), 'null element of frames_u8'),
            'null output 1': (lambda a: a['out_u8'].__setitem__(1, None), 'null element of out_u8'),
            'output is a source': (lambda a: a['out_u8'].__setitem__(1, a['frames_u8'][3]), 'an element of out_u8 overlaps a source frame'),
            'output is the other outputs source': (lambda a: a['out_u8'].__setitem__(0, a['frames_u8'][2]), 'an element of out_u8 overlaps a source frame'),
            # (the frames lie a gap apart: the output ends on the first byte of the next source and touches no other)
            'one byte of the next source': (lambda a: a['out_u8'].__setitem__(0, a['frames_u8'][1] - _out_bytes(a) + 1), 'an element of out_u8 overlaps a source frame'),
            'one byte of the other output': (lambda a: a['out_u8'].__setitem__(0, a['out_u8'][1] - _out_bytes(a) + 1), 'an element of out_u8 overlaps another output'),
            'the same output twice': (lambda a: a['out_u8'].__setitem__(0, a['out_u8'][1]), 'an element of out_u8 overlaps another output')}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(SH, what):
    from ken_burns_effect_amd import _native
    W, H = sc.FRAMES[0]
    change, text = REFUSALS[what]
    rc, got = run(SH, sc.samples_of(W, H, 2).reshape(4, H, W, 3), 2, gap=3 * W * H + 64, change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_shutter_mean_u8: ' + text
    assert (got == 0xFF).all()


def test_on_a_side_stream_behind_a_delay(SH):
    """The entry called raw with the handle of a non-blocking side stream behind stream_gpu's delay: it returns while the delay runs, and the
    result is the twin, bit for bit; the sources hold a decoy until the delay has run out."""
    from ken_burns_effect_amd import _native
    n, S, H, W = 3, 4, 37, 50
    right = torch.from_numpy(_pan(W, H, S, n=n).reshape(n * S, H, W, 3)).cuda()
    decoy = torch.from_numpy(_pan(W, H, S, n=n, seed=60).reshape(n * S, H, W, 3)).cuda()
    frames, out = decoy.clone(), torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')

    def pointers(t):
        return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])

    def call():
        SH._call('kbe_shutter_mean_u8', pointers(frames), n, S, W, H, 3 * W, pointers(out), 3 * W, _native._stream())
        return out
    what = 'shutter_mean_u8'
    got, want = stream_gpu.hold(what, 'bits', [frames], [right], [decoy], call, written=lambda: [out])
    assert what in stream_gpu.ENQUEUED                                      # (the entry had returned while the delay still ran)
    assert np.array_equal(got[0], sc.twin_mean(right.cpu().numpy().reshape(n, S, H, W, 3))) and np.array_equal(got[0], want[0])


def test_shutter_mean_and_its_refusals(SH):
    from ken_burns_effect_amd import _native
    W, H = sc.FRAMES[2]
    samples = _pan(W, H, 8, n=13)
    frames = torch.from_numpy(samples.reshape(13 * 8, H, W, 3)).cuda()
    got = SH.mean(frames, 8)
    assert got.shape == (13, H, W, 3) and got.dtype == torch.uint8 and got.device == frames.device
    assert np.array_equal(got.cpu().numpy(), sc.twin_mean(samples))
    assert torch.equal(SH.mean(frames, 1), frames) and SH.mean(frames, 1).data_ptr() != frames.data_ptr()
    for bad, S in ((frames.cpu(), 8), (frames.int(), 8), (frames[:, :, ::2], 8), (frames[0], 1), (frames[:100], 8), (frames, 33), (frames, 0), (frames[:99], 33)):
        with pytest.raises(_native.KbeError, match=r'shutter\.mean'):
            SH.mean(bad, S)


# -- the route ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    """smoke()'s scene, 128 x 96 with its default windows (the one tests/test_dof_gpu.py renders), 3 steps: the cameras of the steps, the 12
    cameras of Shutter(0.5, 4), and a lens that blurs the scene."""
    from ken_burns_effect_amd import common, dof, shutter, synthetic
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
    open_for = shutter.Shutter(0.5, 4)
    expanded = common.frame_cameras(dict(settings, dblSteps=shutter.sample_steps(settings['dblSteps'], 0.5, 4)), oc)
    assert len(expanded) == 12
    planes = depth.numpy()
    lens = dof.Lens(float(np.percentile(planes, 20)), float(np.percentile(planes, 70)), 12.0, 16)
    return K, settings, oc, cams, expanded, open_for, lens


def _twin(frames, S):
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    return sc.twin_mean(frames.reshape((frames.shape[0] // S, S) + frames.shape[1:]))


def test_render_frames_with_a_shutter_is_the_twin_of_its_samples(SH, scene):
    """Raw, with the crop, and with an out_size 64 wide; fetched and left in HBM; and the calls without a shutter before and after are equal."""
    from ken_burns_effect_amd import common, crop_area
    K, settings, oc, cams, expanded, open_for, lens = scene
    crop, size = common.crop_size(settings), crop_area.size_for(128, 96, width=64)
    before = common.render_frames(cams, oc, None)
    for kw in (dict(crop=None), dict(crop=crop), dict(crop=crop, out_size=size)):
        samples = common.render_frames(expanded, oc, **kw)
        want = _twin(samples, 4)
        assert want.shape == (3,) + samples.shape[1:] and sc.differing_share(samples.reshape((3, 4) + samples.shape[1:]), want) > 0.0, kw      # (no frame is one of its samples)
        fetched = common.render_frames(expanded, oc, shutter=open_for, **kw)
        assert isinstance(fetched, np.ndarray) and np.array_equal(fetched, want), kw
        in_hbm = common.render_frames(expanded, oc, keep_on_device=True, shutter=open_for, **kw)
        assert in_hbm.is_cuda and in_hbm.dtype == torch.uint8 and np.array_equal(in_hbm.cpu().numpy(), want), kw
        assert np.array_equal(common.render_frames(expanded, oc, shutter=tuple(open_for), **kw), want)             # (a plain tuple is taken)
    assert size == (64, 48) and want.shape == (3, 48, 64, 3)
    assert np.array_equal(common.render_frames(cams, oc, None), before)                                        # no state leaks


def test_with_a_lens_every_sample_is_blurred_at_its_frames_focus_depth(SH, scene):
    from ken_burns_effect_amd import common, dof
    K, settings, oc, cams, expanded, open_for, lens = scene
    crop = common.crop_size(settings)
    path = dof.focus_path(lens.focus_from, lens.focus_to, 3)
    repeated = [path[k // 4] for k in range(12)]
    for c in (None, crop):
        samples = common._render_lens(expanded, oc, c, None, True, lens, focus=repeated)
        want = _twin(samples, 4)
        assert np.array_equal(common.render_frames(expanded, oc, c, lens=lens, shutter=open_for), want)
        # (the depths do matter: the lens route's own path over 12 frames gives other bytes)
        assert not np.array_equal(_twin(common.render_frames(expanded, oc, c, keep_on_device=True, lens=lens), 4), want)
    # without the keyword _render_lens does what it did
    assert torch.equal(common._render_lens(cams, oc, None, None, True, lens), common._render_lens(cams, oc, None, None, True, lens, focus=path))


def test_a_shutter_that_blurs_nothing_returns_the_unblurred_routes_bytes(SH, scene):
    """A shutter that is not open (every sample on its frame's own step) and a single sample: the frames of the route without a shutter,
    compared where they lie in HBM."""
    from ken_burns_effect_amd import common, crop_area, shutter
    K, settings, oc, cams, expanded, open_for, lens = scene
    crop, size = common.crop_size(settings), crop_area.size_for(128, 96, width=64)
    for c, s in ((None, None), (crop, None), (crop, size)):
        plain = common.render_frames(cams, oc, c, keep_on_device=True, out_size=s).clone()
        for still in (shutter.Shutter(0.0, 4), shutter.Shutter(0.5, 1)):
            steps = shutter.sample_steps(settings['dblSteps'], *still)
            got = common.render_frames(common.frame_cameras(dict(settings, dblSteps=steps), oc), oc, c, keep_on_device=True, out_size=s, shutter=still)
            assert torch.equal(got, plain), (still, c, s)


def test_more_frames_than_a_chunk(SH, scene):
    """25 steps at S = 8: the route's chunks are 12, 12 and 1 output frames; frames 0, 11, 12 and 24 against the twin of their own samples."""
    from ken_burns_effect_amd import common, shutter
    K, settings, oc, cams, expanded, open_for, lens = scene
    steps = np.linspace(0.0, 1.0, 25).tolist()
    many = common.frame_cameras(dict(settings, dblSteps=shutter.sample_steps(steps, 0.5, 8)), oc)
    got = common.render_frames(many, oc, None, shutter=shutter.Shutter(0.5, 8))
    assert got.shape == (25, 96, 128, 3)
    for i in (0, 11, 12, 24):
        assert np.array_equal(got[i], _twin(common.render_frames(many[8 * i:8 * i + 8], oc, None), 8)[0]), i


def test_process_kenburns_passes_the_shutter_on(SH, scene):
    from ken_burns_effect_amd import common, crop_area
    K, settings, oc, cams, expanded, open_for, lens = scene
    crop, size = common.crop_size(settings), crop_area.size_for(128, 96, width=64)
    frames = common.process_kenburns(settings, oc, None, shutter=open_for)
    assert len(frames) == 3 and np.array_equal(np.stack(frames), _twin(common.render_frames(expanded, oc, crop), 4))
    in_hbm = common.process_kenburns(settings, oc, None, keep_on_device=True, out_size=size, shutter=open_for)
    assert in_hbm.is_cuda and np.array_equal(in_hbm.cpu().numpy(), _twin(common.render_frames(expanded, oc, crop, out_size=size), 4))
    raw = common.process_kenburns(dict(settings, boolCrop=False), oc, None, shutter=open_for)
    assert np.array_equal(np.stack(raw), _twin(common.render_frames(expanded, oc, None), 4))
    assert len(common.process_kenburns(settings, oc, None)) == 3 and settings['dblSteps'] == [0.0, 0.5, 1.0]          # (the caller's settings are not touched)


def _files(directory):
    return sorted(str(p.relative_to(directory)) for p in directory.rglob('*') if p.is_file())


def test_the_pipeline_with_a_shutter_writes_the_files_it_writes_without(SH, tmp_path, monkeypatch):
    """One Pipeline(shutter=0.5, shutter_samples=4, allow_random_weights=True) call on a 64 x 48 image with --write-frames --gif beside one
    without the shutter: the same five files, 3 frames of 48 x 64 x 3, the PNG frames are the returned frames, the GIF has 5 frames, and the
    frames with the shutter differ from those without."""
    from ken_burns_effect_amd import kbe, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES'):
        monkeypatch.delenv(name, raising=False)
    image, _ = synthetic.make_rgbd(48, 64, 12)
    zoom = kbe.windows_for(64, 48, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), False)
    written = {}
    for name, open_for in (('plain', {}), ('shutter', dict(shutter=0.5, shutter_samples=4))):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=3, gif=True, **open_for)
            frames = pipe(image, zoom, str(tmp_path / name))
        assert len(frames) == 3 and all(f.shape == (48, 64, 3) and f.dtype == np.uint8 for f in frames)
        assert _files(tmp_path / name) == ['3d_kbe.gif', '3d_kbe.mp4', 'frames/0.png', 'frames/1.png', 'frames/2.png']
        for i, frame in enumerate(frames):
            png = Image.open(str(tmp_path / name / 'frames' / ('%d.png' % i)))
            assert png.size == (64, 48) and np.array_equal(np.asarray(png.convert('RGB')), frame[:, :, ::-1])
        gif = Image.open(str(tmp_path / name / '3d_kbe.gif'))
        assert gif.size == (64, 48) and gif.n_frames == 5
        written[name] = np.stack(frames)
    assert written['plain'].shape == written['shutter'].shape and not np.array_equal(written['plain'], written['shutter'])
