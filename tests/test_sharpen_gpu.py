"""The output sharpening on the GPU (include/kbe_sharpen.h; kernel: csrc/kbe_sharpen.hip): kbe_sharpen_u8 byte for byte against the NumPy twin
(tests/sharpen_cases.py) under guard bands and both poisons, padded strides, unaligned pointers, the side limits and argument checks, on a side
stream, and the host side built on it (sharpen.apply_sharpen, Pipeline(sharpen=) under a caption, with an enlargement, in a slideshow)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import encoder_gpu as eg
import overlay_cases as oc
import sharpen_cases as sc
import sharpen_gpu as sg
import transition_cases as tc
from test_overlay_gpu import OneRenderPerClip, _files

pytestmark = pytest.mark.gpu
POISONS = (0x00, 0xFF)
ids = lambda v: v if isinstance(v, str) else 'R%d' % v if isinstance(v, int) else '%dx%d' % v                     # noqa: E731


@pytest.fixture(scope='module')
def S():
    from ken_burns_effect_amd import sharpen
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    sharpen.load()
    return sharpen


run = sg.run_sharpen                                   # (the raw call on guarded buffers: tests/sharpen_gpu.py)


def assert_sharpened(S, frames, taps, want, amount=256, threshold=0, poisons=POISONS, **kw):
    n, H, W, _ = np.asarray(frames).shape
    for poison in poisons:
        rc, got = run(S, frames, taps, amount, threshold, poison=poison, **kw)
        assert rc == 0
        assert np.array_equal(got[:, :, :3 * W].reshape(n, H, W, 3), want), (W, H, len(taps) - 1, amount, threshold, poison)
        assert (got[:, :, 3 * W:] == poison).all()                       # the rows' padding is not written


@pytest.mark.parametrize('frame, R', sc.EVERY, ids=ids)
def test_the_device_is_the_twin_byte_for_byte(S, frame, R):
    """37x50, 64x48 and 160x128 frames, 2 frames each, at R = 1, 2, 7 and 24, both poisons.  At R = 24 on 37x50 every tap is clamped on both
    sides and the halo is wider than the frame; 160x128 has three tiles across and four down."""
    W, H = frame
    want = sc.twin_of(W, H, R)
    assert (want != sc.frames(W, H)).any()                              # (the mask does something)
    assert_sharpened(S, sc.frames(W, H), sc.taps_at(R), want)


@pytest.mark.parametrize('threshold', sc.THRESHOLDS)
@pytest.mark.parametrize('amount', sc.AMOUNTS)
def test_amounts_and_thresholds(S, amount, threshold):
    """amount 1, 256 and 1024, threshold 0, 3 and 255 at R = 2 on 37x50 (odd sides, one tile) and at R = 7 on 160x128."""
    for (W, H), R in (((37, 50), 2), ((160, 128), 7)):
        want = sc.twin_of(W, H, R, amount, threshold)
        if threshold == 255:
            assert np.array_equal(want, sc.frames(W, H))                # (no difference reaches 255 counts)
        assert_sharpened(S, sc.frames(W, H), sc.taps_at(R), want, amount, threshold, poisons=(0xFF,))


@pytest.mark.parametrize('frame', sc.THIN, ids=ids)
def test_thin_frames(S, frame):
    """1x1, 1x40 and 40x1 at R = 1, 7 and 24: the border pixel is every tap along the thin axis; a 1x1 frame is its own output."""
    W, H = frame
    frames = sc.thin(W, H)
    for R in (1, 7, 24):
        want = sc.twin_sharpen(frames, sc.taps_at(R), 1024)
        if frame == (1, 1):
            assert np.array_equal(want, frames)
        assert_sharpened(S, frames, sc.taps_at(R), want, 1024)


def test_many_tiles_across_and_down(S):
    """700x20: eleven tiles across, each staging its own span of the rows and its neighbours' pixels; its transpose, 20x700: 22 tiles down."""
    frame = sc.wide()
    tall = np.ascontiguousarray(frame.transpose(0, 2, 1, 3))
    for R in (2, 24):
        assert_sharpened(S, frame, sc.taps_at(R), sc.twin_sharpen(frame, sc.taps_at(R), 512), 512, poisons=(0xFF,))
        assert_sharpened(S, tall, sc.taps_at(R), sc.twin_sharpen(tall, sc.taps_at(R), 512), 512, poisons=(0x00,))


@pytest.mark.parametrize('frame', [(65535, 1), (1, 65535)], ids=ids)
def test_the_side_limit(S, frame):
    """One 65535x1 frame and one 1x65535 frame at R = 24: the longest sides there are, 1024 tiles across and 2048 down; one more is refused
    with the output untouched."""
    from ken_burns_effect_amd import _native
    W, H = frame
    picture = np.ascontiguousarray(eg.tiled(H, W, 7)[None])
    assert picture.shape == (1, H, W, 3)
    assert_sharpened(S, picture, sc.taps_at(24), sc.twin_sharpen(picture, sc.taps_at(24), 700), 700, poisons=(0xFF,))
    change = (lambda a: a.update(W=65536, stride_bytes=3 * 65536, out_stride_bytes=3 * 65536)) if H == 1 else (lambda a: a.update(H=65536))
    rc, got = run(S, picture, sc.taps_at(24), change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_sharpen_u8: W or H outside 1..65535'
    assert (got == 0xFF).all()


@pytest.mark.parametrize('n', [1, 12, 13])
def test_the_launch_split(S, n):
    """At most twelve frames a launch: 1, 12, and 13 that take two."""
    W, H = sc.FRAMES[1]
    assert_sharpened(S, sc.frames(W, H, n), sc.taps_at(7), sc.twin_of(W, H, 7, 300, 1, n), 300, 1, poisons=(0xFF,))


@pytest.mark.parametrize('R', [1, 7, 24], ids=ids)
def test_padded_strides_and_unaligned_pointers(S, R):
    """Source rows 7 bytes apart beyond their pixels (every row at another alignment), output rows 5, the source and the output 1, 2 and 3
    bytes off their allocations: the twin's bytes, the padding of every row and the bands around every frame untouched."""
    for W, H in (sc.FRAMES[0], sc.FRAMES[2]):
        want = sc.twin_of(W, H, R)
        assert_sharpened(S, sc.frames(W, H), sc.taps_at(R), want, pad=7, out_pad=5, shift=3, src_shift=1)
        assert_sharpened(S, sc.frames(W, H), sc.taps_at(R), want, pad=1, out_pad=0, shift=1, src_shift=2, poisons=(0xFF,))
        assert_sharpened(S, sc.frames(W, H), sc.taps_at(R), want, pad=0, out_pad=2, shift=2, src_shift=3, poisons=(0x00,))


def _taps(values):
    return (ctypes.c_uint16 * len(values))(*values)


REFUSALS = {'null frames': (lambda a: a.update(frames_u8=None), 'null frames_u8'),
            'null out': (lambda a: a.update(out_u8=None), 'null out_u8'),
            'null taps': (lambda a: a.update(taps=None), 'null taps'),
            'null frame 0': (lambda a: a['frames_u8'].__setitem__(0, None), 'null element of frames_u8'),
            'null output 1': (lambda a: a['out_u8'].__setitem__(1, None), 'null element of out_u8'),
            'n = 0': (lambda a: a.update(n_frames=0), 'n_frames < 1'),
            'W = 0': (lambda a: a.update(W=0), 'W or H outside 1..65535'),
            'H = 65536': (lambda a: a.update(H=65536), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'out stride < 3 W': (lambda a: a.update(out_stride_bytes=3 * a['W'] - 1), 'out_stride_bytes < 3 W'),
            'radius = 0': (lambda a: a.update(radius=0), 'radius outside 1..24'),
            'radius = 25': (lambda a: a.update(radius=25), 'radius outside 1..24'),
            'taps one short': (lambda a: a.update(taps=_taps((32514, 126))), 'taps[0] + 2 (taps[1] + .. + taps[radius]) is not 32768'),
            'taps one over': (lambda a: a.update(taps=_taps((32768, 1))), 'taps[0] + 2 (taps[1] + .. + taps[radius]) is not 32768'),
            'amount = 0': (lambda a: a.update(amount=0), 'amount outside 1..1024'),
            'amount = 1025': (lambda a: a.update(amount=1025), 'amount outside 1..1024'),
            'threshold = -1': (lambda a: a.update(threshold=-1), 'threshold outside 0..255'),
            'threshold = 256': (lambda a: a.update(threshold=256), 'threshold outside 0..255')}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(S, what):
    from ken_burns_effect_amd import _native
    W, H = sc.FRAMES[0]
    change, text = REFUSALS[what]
    rc, got = run(S, sc.frames(W, H), sc.taps_at(1), change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_sharpen_u8: ' + text
    assert (got == 0xFF).all()


def test_on_a_side_stream(S):
    """As tests/test_streams_gpu.py holds the other filters: the raw call with a side stream's handle behind a delay, the right frames copied
    over the decoy only behind that delay; bit for bit what the default stream gives."""
    import stream_gpu
    n, (W, H) = 3, (50, 37)
    taps = sc.taps_at(7)
    rng = np.random.default_rng(3)
    right, decoy = (torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda() for _ in range(2))
    frames, out = decoy.clone(), torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
    pointers = lambda t: (ctypes.c_void_p * len(t))(*[t[i].data_ptr() for i in range(len(t))])         # noqa: E731

    def call():
        S._call('kbe_sharpen_u8', pointers(frames), n, W, H, 3 * W, pointers(out), 3 * W, _taps(taps), 7, 256, 0, sg.stream())
        return out
    got, want = stream_gpu.hold('sharpen_u8', 'bits', [frames], [right], [decoy], call, written=lambda: [out])
    assert np.array_equal(want[0], sc.twin_sharpen(right.cpu().numpy(), taps))


def test_apply_sharpen_is_the_twin_and_in_place(S):
    """13 frames: two groups through one scratch tensor of 12; the tensor given is the tensor returned, and holds the twin."""
    from ken_burns_effect_amd import _native
    W, H = sc.FRAMES[2]
    host = np.array(sc.frames(W, H, 13))
    frames = torch.from_numpy(host.copy()).cuda()
    at = frames.data_ptr()
    request = S.request('1.5,2.3,2', environment=False)
    assert request == {'amount': 384, 'sigma': 2.3, 'threshold': 2, 'taps': sc.taps_at(7), 'radius': 7}
    got = S.apply_sharpen(frames, request)
    assert got is frames and frames.data_ptr() == at and np.array_equal(frames.cpu().numpy(), sc.twin_sharpen(host, sc.taps_at(7), 384, 2))
    before = frames.clone()
    for bad in (frames.cpu(), frames.int(), frames[0], frames[:, :, ::2], None):
        with pytest.raises(_native.KbeError, match=r'sharpen\.apply_sharpen'):
            S.apply_sharpen(bad, request)
    assert torch.equal(frames, before)


# -- the routes ----------------------------------------------------------------------------------
ENV = ('KBE_WIDTH', 'KBE_ENLARGE', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER',
       'KBE_SHUTTER_SAMPLES', 'KBE_Y4M', 'KBE_OVERLAY', 'KBE_OVERLAY_AT', 'KBE_OVERLAY_OPACITY', 'KBE_CAPTION', 'KBE_CAPTION_AT', 'KBE_CAPTION_SIZE', 'KBE_LUT', 'KBE_GRADE', 'KBE_LOOK',
       'KBE_LUT_STRENGTH', 'KBE_SHARPEN')


def test_the_sharpening_of_a_pipeline_and_of_a_slideshow(S, tmp_path, monkeypatch):
    """One Pipeline (seeded weights, 6 steps, --write-frames) and two synthetic 64 x 48 photos, every clip rendered once (OneRenderPerClip: two
    renders of one cloud need not agree to the byte, their fp32 sums' order is the atomics', so both calls are given ONE set of frames).
    With sharpen='1.5,0.6,1' the Pipeline asks for the frames it asks for without it, left in HBM, and returns the twin of them; with a
    caption, the caption's twin on the sharpened frames -- the caption is not sharpened; the PNG frames decode to those frames and the GIF is
    written; Pipeline.render and KBE_SHARPEN give the same; with width=100 and enlarge the enlarged frames are sharpened.  A slideshow of the
    two photos with T = 2 is the join of the sharpened clips.  A Pipeline call without the option writes the same bytes before and after."""
    from ken_burns_effect_amd import kbe, overlay, pipeline, slideshow, synthetic, transition
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    images = [synthetic.make_rgbd(48, 64, seed)[0] for seed in (12, 13)]
    zoom = kbe.windows_for(64, 48, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=6)
    once = OneRenderPerClip(pipeline.common.process_kenburns)
    monkeypatch.setattr(pipeline.common, 'process_kenburns', once)
    before = pipe(images[0], zoom, str(tmp_path / 'before'))
    plain = np.stack(before)
    assert len(once.rendered) == 1 and once.on_device == [False]

    # the option alone
    taps = sc.taps_at(2)
    pipe.sharpen = '1.5,0.6,1'
    crisp = sc.twin_sharpen(plain, taps, 384, 1)
    assert (crisp != plain).mean() > 0.1
    got = np.stack(pipe(images[0], zoom, None))
    assert len(once.rendered) == 1 and once.calls[1] == once.calls[0] and once.on_device == [False, True]            # (the same frames, asked to stay in HBM)
    assert np.array_equal(got, crisp)
    pipe.sharpen = (1.5, 0.6, 1)
    assert np.array_equal(np.stack(pipe(images[0], zoom, None)), crisp)
    pipe.sharpen = None
    monkeypatch.setenv('KBE_SHARPEN', '1.5,0.6,1')
    assert np.array_equal(np.stack(pipe(images[0], zoom, None)), crisp)
    monkeypatch.delenv('KBE_SHARPEN')

    # under a caption, with every output
    pipe.sharpen, pipe.caption, pipe.caption_at, pipe.caption_size, pipe.overlay_margin, pipe.gif = '1.5,0.6,1', 'A view', 'top-right', 8, 2, True
    got = np.stack(pipe(images[0], zoom, str(tmp_path / 'crisp')))
    text = overlay.caption_image('A view', 8)
    cx, cy = overlay.place('top-right', 64, 48, text.shape[1], text.shape[0], 2)
    want = oc.twin_over(crisp, text, cx, cy, 256)
    assert np.array_equal(got, want) and len(once.rendered) == 1
    assert not np.array_equal(want, sc.twin_sharpen(oc.twin_over(plain, text, cx, cy, 256), taps, 384, 1))              # (the caption is not sharpened)
    files = _files(tmp_path / 'crisp')
    assert sorted(files) == sorted(['3d_kbe.mp4', '3d_kbe.gif'] + ['frames/%d.png' % i for i in range(6)])
    for i in range(6):
        png = Image.open(str(tmp_path / 'crisp' / 'frames' / ('%d.png' % i)))
        assert png.size == (64, 48) and np.array_equal(np.asarray(png.convert('RGB')), want[i][:, :, ::-1])
    assert Image.open(str(tmp_path / 'crisp' / '3d_kbe.gif')).n_frames == 11
    pipe.gif = None
    rendered = pipe.render(images[0], zoom)
    assert rendered.is_cuda and np.array_equal(rendered.cpu().numpy(), want) and once.calls[-1] == once.calls[0] and len(once.rendered) == 1
    pipe.caption = pipe.caption_at = pipe.caption_size = pipe.overlay_margin = None

    # after the enlargement: the crop of 57 x 43 to 100 x 75, then the mask
    pipe.sharpen, pipe.width, pipe.enlarge = None, 100, True
    grown = np.stack(pipe(images[0], zoom, None))
    assert grown.shape == (6, 75, 100, 3) and len(once.rendered) == 2
    pipe.sharpen = '1.5,0.6,1'
    assert np.array_equal(np.stack(pipe(images[0], zoom, None)), sc.twin_sharpen(grown, taps, 384, 1)) and len(once.rendered) == 2 and once.calls[-1] == once.calls[-2]
    pipe.width = pipe.enlarge = None

    # refused before a network runs: nothing more was asked of process_kenburns
    asked = len(once.calls)
    pipe.sharpen = '5'
    with pytest.raises(ValueError, match=r'^--sharpen 5: AMOUNT 5: above 0 and at most 4$'):
        pipe(images[0], zoom, str(tmp_path / 'refused'))
    with pytest.raises(ValueError, match=r'^--sharpen 5: AMOUNT 5: above 0 and at most 4$'):
        pipe.render(images[0], zoom)
    with pytest.raises(ValueError, match=r'^--sharpen 5: AMOUNT 5: above 0 and at most 4$'):
        slideshow.make(images, str(tmp_path / 'refused'), pipe, 'dissolve', 2)
    assert len(once.calls) == asked and not (tmp_path / 'refused').exists()

    # a slideshow: the clips sharpened by Pipeline.render, the transition blends sharpened frames
    pipe.sharpen = None
    clips = [pipe.render(image, zoom).cpu().numpy() for image in images]
    assert np.array_equal(clips[0], plain) and len(once.rendered) == 3
    pipe.sharpen = '1.5,0.6,1'
    show = slideshow.make(images, str(tmp_path / 'show'), pipe, 'dissolve', 2)
    assert len(once.rendered) == 3
    fine = [sc.twin_sharpen(clip, taps, 384, 1) for clip in clips]
    blend = transition.progress_table(2)
    joined = np.stack([fine[0][i] for i in range(4)] + [tc.twin_blend(fine[0][4 + j][None], fine[1][j][None], 'dissolve', [blend[j]])[0] for j in range(2)] + [fine[1][i] for i in range(2, 6)])
    assert len(show) == 10 and np.array_equal(np.stack(show), joined) and not np.array_equal(fine[0], clips[0])
    pipe.sharpen = None

    # without the option: the same bytes as before
    pipe(images[0], zoom, str(tmp_path / 'after'))
    assert once.calls[-1] == once.calls[0] and once.on_device[-1] is False and len(once.rendered) == 3
    assert _files(tmp_path / 'after') == _files(tmp_path / 'before') and sorted(_files(tmp_path / 'before')) == ['3d_kbe.mp4'] + ['frames/%d.png' % i for i in range(6)]
