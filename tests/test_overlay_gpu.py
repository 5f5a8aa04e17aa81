"""The overlay on the GPU (include/kbe_overlay.h; kernel: csrc/kbe_overlay.hip): kbe_overlay_u8 byte for byte against the NumPy twin
(tests/overlay_cases.py) under guard bands and both poisons, the whole of every frame compared -- the entry works in place, so what lies
outside the clipped rectangle has to be what it was --, at the shapes where the kernel can go wrong: clipping off every edge and corner,
rectangles narrower than a piece, rows around a workgroup's span, every combination of alignment classes, the cut into launches; every
refusal, a side stream, and the host side built on it (overlay.apply, Pipeline's two layers, a slideshow's captions)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import overlay_cases as oc
import overlay_gpu as og
import stream_gpu
import transition_cases as tc

pytestmark = pytest.mark.gpu
run, assert_over = og.run_overlay, og.assert_over


@pytest.fixture(scope='module')
def OV():
    from ken_burns_effect_amd import overlay
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    overlay.load()
    return overlay


# -- the entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize('frame', oc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(OV, frame):
    """37x50, 64x48 and 160x128 frames with a 21x9 overlay whose alpha holds 0, 255 and what lies between; two frames in one call at different
    x, y and opacity; the frames' rows padded by 4, the overlay's by 3."""
    W, H = frame
    frames, picture = oc.frames_of(W, H), oc.overlay_of(*oc.OVERLAY)
    want = oc.twin_of(W, H)
    assert {0, 255} <= set(np.unique(picture[:, :, 3]).tolist()) and len(np.unique(picture[:, :, 3])) > 100
    assert not np.array_equal(want, frames) and not np.array_equal(want[0] != frames[0], want[1] != frames[1])
    assert all((want[i] != frames[i]).any(axis=2).sum() > 21 * 9 // 2 for i in (0, 1))
    assert_over(OV, frames, picture, oc.X, oc.Y, oc.OPACITY, want, pad=4, overlay_pad=3)


CLIPS = {'left': (-5, 3), 'right': (30, 3), 'top': (3, -4), 'bottom': (3, 45), 'top-left': (-5, -4), 'top-right': (30, -4), 'bottom-left': (-5, 45), 'bottom-right': (30, 45),
         'one pixel at the far corner': (36, 49), 'one pixel at the near corner': (-20, -8)}
OUTSIDE = {'x = W': (37, 3), 'x = -w': (-21, 3), 'y = H': (3, 50), 'y = -h': (3, -9), 'far away': (65535, -65535), 'past both': (40, 60)}


@pytest.mark.parametrize('where', sorted(CLIPS))
def test_clipped_at_every_edge_and_corner(OV, where):
    """A 21x9 overlay off each edge and each corner of a 37x50 frame, in two frames of a call: the second at the opposite place.  The clipped
    part shows, and nothing else changes."""
    frames, picture = oc.frames_of(37, 50), oc.overlay_of(*oc.OVERLAY)
    x, y = CLIPS[where]
    xs, ys = (x, 37 - 21 - x), (y, 50 - 9 - y)
    want = oc.twin_over(frames, picture, xs, ys, (256, 99))
    assert (want[0] != frames[0]).any() or where.startswith('one pixel')
    assert_over(OV, frames, picture, xs, ys, (256, 99), want, pad=1, shift=3, overlay_pad=2, overlay_shift=1)


def test_wholly_outside_leaves_the_frame_as_it_is(OV):
    """Exactly touching -- x = W, x = -w, y = H, y = -h --, further out, and at the limit of the positions: the frames are what they were."""
    frames, picture = oc.frames_of(37, 50, 6), oc.overlay_of(*oc.OVERLAY, alpha=255)
    xs, ys = zip(*[OUTSIDE[k] for k in sorted(OUTSIDE)])
    assert_over(OV, frames, picture, xs, ys, 256, frames, pad=2)
    # one of them inside: that frame alone changes
    xs, ys = list(xs), list(ys)
    xs[2], ys[2] = 36, 49
    want = assert_over(OV, frames, picture, xs, ys, 256, None, pad=2)
    assert [np.array_equal(want[i], frames[i]) for i in range(6)] == [True, True, False, True, True, True]


def test_an_overlay_larger_than_the_frame(OV):
    """An 80x70 overlay over all of a 37x50 frame at negative x and y, and over all of a 64x48 one but its last column and row."""
    big = oc.overlay_of(80, 70, alpha=None)
    for (W, H), x, y in (((37, 50), (-13, -43), (-7, -20)), ((64, 48), (-15, -17), (-21, -23))):
        frames = oc.frames_of(W, H)
        want = oc.twin_over(frames, big, x, y, (256, 201))
        assert (want != frames).any(axis=3).mean() > 0.5
        assert_over(OV, frames, big, x, y, (256, 201), want, pad=3, overlay_pad=1, shift=5, overlay_shift=2)
    frames = oc.frames_of(64, 48)
    want = assert_over(OV, frames, big, -17, -23, 256, None)
    assert np.array_equal(want[:, -1], frames[:, -1]) and np.array_equal(want[:, :, -1], frames[:, :, -1])


@pytest.mark.parametrize('shape', [(1, 9), (2, 9), (5, 9), (21, 1), (1, 1)], ids=lambda v: '%dx%d' % v)
def test_narrow_overlays(OV, shape):
    """w = 1, 2 and 5: a rectangle's row shorter than one 16-byte piece, which an unaligned row still cuts in two; h = 1; one pixel.  At sixteen
    places in a row, so that the rectangle begins at every byte of a piece."""
    w, h = shape
    frames, picture = oc.frames_of(37, 20, 16), oc.overlay_of(w, h, alpha=None)
    xs, ys = list(range(3, 19)), [(5 * i) % 11 for i in range(16)]
    want = oc.twin_over(frames, picture, xs, ys, 230)
    assert_over(OV, frames, picture, xs, ys, 230, want, pad=0, overlay_pad=1, overlay_shift=3)
    assert_over(OV, frames, picture, xs, ys, 230, want, pad=2, shift=7)


@pytest.mark.parametrize('frame', [(1, 7), (1366, 3)], ids=lambda v: '%dx%d' % v)
def test_narrow_and_wide_frames(OV, frame):
    """W = 1: rows of three bytes under an overlay that is clipped to one column.  1366 x 3 with an overlay as wide as the frame: rows of 4098
    bytes, two bytes beyond four spans."""
    W, H = frame
    frames, picture = oc.frames_of(W, H), oc.overlay_of(W if W > 1 else 5, 2)
    xs = (0, 0) if W > 1 else (0, -3)
    for kw in (dict(), dict(pad=3, shift=13, overlay_pad=2, overlay_shift=1)):
        want = assert_over(OV, frames, picture, xs, (0, 1), (256, 77), None, **kw)
        assert (want != frames).any()


@pytest.mark.parametrize('end', [og.SPAN - 1, og.SPAN, og.SPAN + 1])
def test_rows_around_a_workgroups_span(OV, end):
    """A workgroup takes SPAN = 1024 bytes of a rectangle's row, counted from the address of the row's first byte rounded down to 16.  An overlay
    of 341 pixels, 1023 bytes of a frame's row, at x = 2 of a 345-pixel frame whose stride is 1040, a multiple of 16: with the frame 10, 11 and
    12 bytes off its allocation every row of the rectangle begins 0, 1 and 2 bytes into a piece and ends one byte short of the span, exactly on
    it, and one byte beyond it, in a second workgroup whose only piece is one byte.  5 rows: a second workgroup down the rectangle as well."""
    W, H, w = 345, 7, 341
    assert og.SPAN == 1024 and 3 * w == og.SPAN - 1 and (3 * W + 5) % 16 == 0
    shift = end - 3 * w + 10
    assert (shift + 3 * 2) % 16 + 3 * w == end
    frames, picture = oc.frames_of(W, H, 1), oc.overlay_of(w, 5, alpha=255)
    want = oc.twin_over(frames, picture, 2, 1, 256)
    assert np.array_equal(want[0, 1:6, 2:343], picture[:, :, :3]) and np.array_equal(want[0, :, 343:], frames[0, :, 343:])
    assert_over(OV, frames, picture, 2, 1, 256, want, pad=5, shift=shift, overlay_shift=3, aligned=True)
    assert_over(OV, frames, oc.overlay_of(w, 5), 2, 1, 131, None, pad=5, shift=shift, overlay_pad=3, aligned=True)


@pytest.mark.parametrize('shift', range(16))
def test_every_combination_of_alignment_classes(OV, shift):
    """40 x 20 frames whose rows lie 121 bytes apart, an odd number, so that a frame's rows walk through all sixteen classes of their address,
    the frame `shift` bytes off its allocation; a 9 x 17 overlay whose rows lie 37 bytes apart, so that its rows walk through all four
    classes of theirs, shift / 4 bytes off its allocation; sixteen frames in a call, frame i with the overlay at x = i.  The sixteen calls
    reach all 1024 combinations of (frame row address mod 16, overlay row address mod 4, x): with them every byte of a piece at which a
    rectangle's row can begin, at every class of the overlay, and every channel at which a piece can begin."""
    W, H, w, h, n = 40, 20, 9, 17, 16
    stride, overlay_stride = 3 * W + 1, 4 * w + 1
    triples = {((s + stride * Y) % 16, (s // 4 + overlay_stride * (Y - 1)) % 4, i) for s in range(16) for i in range(n) for Y in range(1, 1 + h)}
    assert len(triples) == 16 * 4 * 16
    leads = {((a + 3 * i) % 16, b) for a, b, i in triples}
    assert len(leads) == 16 * 4
    frames, picture = oc.frames_of(W, H, n), oc.overlay_of(w, h)
    want = oc.twin_over(frames, picture, list(range(n)), 1, 256)
    assert_over(OV, frames, picture, list(range(n)), 1, 256, want, pad=1, shift=shift, overlay_pad=1, overlay_shift=shift // 4, aligned=True)


def test_the_extremes(OV):
    """Alpha 0 everywhere: the frames as they were.  Alpha 255 at opacity 256: the overlay's bytes.  Opacity 0 over alpha 255: the frames as
    they were.  Frames and overlay all 0 and all 255 at opacity 1, 128 and 255."""
    W, H = 37, 12
    frames = oc.frames_of(W, H, 3)
    clear, solid = oc.overlay_of(21, 9, alpha=0), oc.overlay_of(21, 9, alpha=255)
    assert_over(OV, frames, clear, 4, 2, (256, 255, 1), frames, pad=1)
    want = assert_over(OV, frames, solid, 4, 2, 256, None, pad=1)
    assert all(np.array_equal(want[i, 2:11, 4:25], solid[:, :, :3]) for i in range(3))
    assert_over(OV, frames, solid, 4, 2, 0, frames, shift=1)
    want = assert_over(OV, frames, solid, 4, 2, (0, 256, 0), None)
    assert np.array_equal(want[0], frames[0]) and np.array_equal(want[2], frames[2]) and not np.array_equal(want[1], frames[1])
    white, black = np.full((3, H, W, 3), 255, np.uint8), np.zeros((3, H, W, 3), np.uint8)
    for alpha in (255, 128, 1):
        over_white, over_black = np.full((9, 21, 4), 255, np.uint8), np.zeros((9, 21, 4), np.uint8)
        over_white[:, :, 3] = over_black[:, :, 3] = alpha
        for frames_, picture in ((white, over_black), (black, over_white), (white, over_white), (black, over_black)):
            assert_over(OV, frames_, picture, (0, 16, -3), (0, 3, 8), (1, 128, 255), None, pad=2, overlay_shift=2)
    assert int(oc.over(0, 255, oc.effective(255, 128))) == 128 and int(oc.over(255, 0, oc.effective(255, 1))) == 254 and int(oc.over(0, 255, oc.effective(255, 255))) == 254


def test_the_cut_into_launches(OV):
    """A launch carries 12 frames: 13 frames with 13 places and opacities are 12 + 1, every frame changed in its own way; with the tables rotated
    every frame comes out another.  Frames that are in no launch -- opacity 0, a rectangle that is empty -- do not count: 12 of those and 13
    that are make 25 frames in two launches."""
    W, H, n = 40, 16, OV.FRAMES_PER_LAUNCH + 1
    assert n == 13
    frames, picture = oc.frames_of(W, H, n), oc.overlay_of(*oc.OVERLAY)
    xs, ys, opacities = [2 * i - 3 for i in range(n)], [(5 * i) % 9 - 1 for i in range(n)], [40 + 18 * i for i in range(n)]
    want = oc.twin_over(frames, picture, xs, ys, opacities)
    rotated = oc.twin_over(frames, picture, xs[1:] + xs[:1], ys[1:] + ys[:1], opacities[1:] + opacities[:1])
    assert all(not np.array_equal(want[i], frames[i]) and not np.array_equal(rotated[i], want[i]) for i in range(n))
    assert_over(OV, frames, picture, xs, ys, opacities, want, pad=1)
    more = oc.frames_of(W, H, 25)
    xs, ys, opacities = [3] * 25, [2] * 25, [200] * 25
    for i in range(0, 24, 2):
        (opacities if i % 4 else xs)[i] = 0 if i % 4 else W
    want = assert_over(OV, more, picture, xs, ys, opacities, None, poisons=(0xFF,))
    assert sum(not np.array_equal(want[i], more[i]) for i in range(25)) == 13


def _frame_bytes(a):
    return (a['H'] - 1) * a['stride_bytes'] + 3 * a['W']


def _overlay_bytes(a):
    return (a['h'] - 1) * a['overlay_stride_bytes'] + 4 * a['w']


OVERLAPS_FRAME, OVERLAPS_OVERLAY = 'an element of frames_u8 overlaps another frame', 'an element of frames_u8 overlaps the overlay'
REFUSALS = {'null frames': (lambda a: a.update(frames_u8=None), 'null frames_u8'), 'null overlay': (lambda a: a.update(overlay_rgba=None), 'null overlay_rgba'),
            'null x': (lambda a: a.update(x=None), 'null x'), 'null y': (lambda a: a.update(y=None), 'null y'), 'null opacity': (lambda a: a.update(opacity=None), 'null opacity'),
            'n = 0': (lambda a: a.update(n=0), 'n < 1'), 'n = -1': (lambda a: a.update(n=-1), 'n < 1'),
            'W = 65536': (lambda a: a.update(W=65536, stride_bytes=3 * 65536), 'W or H outside 1..65535'), 'H = 0': (lambda a: a.update(H=0), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'w = 0': (lambda a: a.update(w=0), 'w or h outside 1..65535'), 'h = 65536': (lambda a: a.update(h=65536), 'w or h outside 1..65535'),
            'overlay stride < 4 w': (lambda a: a.update(overlay_stride_bytes=4 * a['w'] - 1), 'overlay_stride_bytes < 4 w'),
            'null frame 1': (lambda a: a['frames_u8'].__setitem__(1, None), 'null element of frames_u8'),
            'x 65536': (lambda a: a['x'].__setitem__(1, 65536), 'an element of x outside -65535..65535'),
            'x -65536': (lambda a: a['x'].__setitem__(0, -65536), 'an element of x outside -65535..65535'),
            'y 65536': (lambda a: a['y'].__setitem__(0, 65536), 'an element of y outside -65535..65535'),
            'y -65536': (lambda a: a['y'].__setitem__(1, -65536), 'an element of y outside -65535..65535'),
            'opacity 257': (lambda a: a['opacity'].__setitem__(1, 257), 'an element of opacity outside 0..256'),
            'opacity -1': (lambda a: a['opacity'].__setitem__(0, -1), 'an element of opacity outside 0..256'),
            'the same frame twice': (lambda a: a['frames_u8'].__setitem__(1, a['frames_u8'][0]), OVERLAPS_FRAME),
            'one byte of the other frame': (lambda a: a['frames_u8'].__setitem__(0, a['frames_u8'][1] - _frame_bytes(a) + 1), OVERLAPS_FRAME),
            'the overlay is a frame': (lambda a: a.update(overlay_rgba=a['frames_u8'][1]), OVERLAPS_OVERLAY),
            'the overlay on a frames last byte': (lambda a: a.update(overlay_rgba=a['frames_u8'][0] + _frame_bytes(a) - 1), OVERLAPS_OVERLAY),
            'a frame on the overlays last byte': (lambda a: a['frames_u8'].__setitem__(1, a['overlay_rgba'] + _overlay_bytes(a) - 1), OVERLAPS_OVERLAY)}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_frames_untouched(OV, what):
    from ken_burns_effect_amd import _native
    W, H = oc.FRAMES[0]
    change, text = REFUSALS[what]
    frames = oc.frames_of(W, H)
    rc, got = run(OV, frames, oc.overlay_of(*oc.OVERLAY, alpha=255), oc.X, oc.Y, oc.OPACITY, pad=2, change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_overlay_u8: ' + text
    assert np.array_equal(got[:, :, :3 * W].reshape(2, H, W, 3), frames) and (got[:, :, 3 * W:] == 0xFF).all()


def test_frames_that_touch_are_taken(OV):
    """Frames back to back in one tensor -- the next begins with the byte behind the last -- are no overlap."""
    frames = torch.from_numpy(oc.frames_of(37, 50, 3).copy()).cuda()
    picture = torch.from_numpy(oc.overlay_of(*oc.OVERLAY).copy()).cuda()
    got = OV.apply(frames, picture, (-3, 20, 5), (45, -2, 7), (256, 100, 3))
    assert got is frames and np.array_equal(got.cpu().numpy(), oc.twin_over(oc.frames_of(37, 50, 3), oc.overlay_of(*oc.OVERLAY), (-3, 20, 5), (45, -2, 7), (256, 100, 3)))


def _pointers(t):
    return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])


def test_on_a_side_stream_behind_a_delay(OV):
    """The entry called raw with the handle of a non-blocking side stream behind stream_gpu's delay: it returns while the delay runs, and the
    result is the twin, bit for bit; the frames and the overlay hold a decoy until the delay has run out."""
    from ken_burns_effect_amd import _native
    n, H, W, w, h = 13, 37, 50, 33, 21
    right = [torch.from_numpy(oc.frames_of(W, H, n).copy()).cuda(), torch.from_numpy(oc.overlay_of(w, h, alpha=255).copy()).cuda()]
    decoy = [torch.from_numpy(oc.frames_of(W, H, n, 150).copy()).cuda(), torch.from_numpy(oc.overlay_of(w, h, 9, alpha=255).copy()).cuda()]
    frames, picture = [t.clone() for t in decoy]
    xs, ys, opacities = [i - 2 for i in range(n)], [2 * i - 4 for i in range(n)], [256 - 9 * i for i in range(n)]

    def call():
        OV._call('kbe_overlay_u8', _pointers(frames), n, W, H, 3 * W, picture.data_ptr(), w, h, 4 * w, (ctypes.c_int32 * n)(*xs), (ctypes.c_int32 * n)(*ys),
                 (ctypes.c_int32 * n)(*opacities), _native._stream())
        return frames
    what = 'overlay_u8'
    got, want = stream_gpu.hold(what, 'bits', [frames, picture], right, decoy, call)
    assert what in stream_gpu.ENQUEUED                                      # (the entry had returned while the delay still ran)
    assert np.array_equal(got[0], oc.twin_over(right[0].cpu().numpy(), right[1].cpu().numpy(), xs, ys, opacities)) and np.array_equal(got[0], want[0])


# -- the module ----------------------------------------------------------------------------------
def test_apply_and_its_refusals(OV):
    from ken_burns_effect_amd import _native
    W, H = oc.FRAMES[2]
    n = 13
    host, picture = oc.frames_of(W, H, n), oc.overlay_of(*oc.OVERLAY)
    frames, layer = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(picture.copy()).cuda()
    got = OV.apply(frames, layer, 100, 60)
    assert got is frames and np.array_equal(got.cpu().numpy(), oc.twin_over(host, picture, 100, 60, 256))
    frames.copy_(torch.from_numpy(host.copy()))
    xs, ys, opacities = list(range(-6, 7)), [10 * i for i in range(n)], OV.opacity_table(n, 1, 12, 4)
    assert np.array_equal(OV.apply(frames, layer, xs, ys, opacities).cpu().numpy(), oc.twin_over(host, picture, xs, ys, opacities))
    before = frames.clone()
    for args in ((frames.cpu(), layer, 0, 0), (frames, layer.cpu(), 0, 0), (frames.int(), layer, 0, 0), (frames[0], layer, 0, 0), (frames[:, :, ::2], layer, 0, 0),
                 (frames, layer[:, :, :3], 0, 0), (frames, layer[None], 0, 0), (frames, layer.int(), 0, 0), (frames, layer[:, ::2], 0, 0), (frames, None, 0, 0), (None, layer, 0, 0),
                 (frames, layer, [0] * 12, 0), (frames, layer, 0, [0] * 14), (frames, layer, 0.5, 0), (frames, layer, 0, 0, 257), (frames, layer, 0, 0, -1), (frames, layer, 0, 0, [256] * 12),
                 (frames, layer, 65536, 0), (frames, layer, 0, -65536), (frames, layer, 0, 0, None), (frames, layer, 'left', 0), (frames, frames[0].view(H, -1, 4), 0, 0)):
        with pytest.raises(_native.KbeError, match=r'overlay\.apply|kbe_overlay_u8: an element of frames_u8 overlaps the overlay'):
            OV.apply(*args)
    assert torch.equal(frames, before)


# -- the routes ----------------------------------------------------------------------------------
ENV = ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES', 'KBE_Y4M',
       'KBE_OVERLAY', 'KBE_OVERLAY_AT', 'KBE_OVERLAY_OPACITY', 'KBE_CAPTION', 'KBE_CAPTION_AT', 'KBE_CAPTION_SIZE')


def _files(directory):
    return {str(p.relative_to(directory)): p.read_bytes() for p in sorted(directory.rglob('*')) if p.is_file()}


class OneRenderPerClip:
    """common.process_kenburns as the pipeline module sees it, with a memory: the first call for a photo (the bytes of objectCommon's image), a
    camera path, an output size, a lens and a shutter renders -- once, into HBM --, and every later call with the same arguments gets those
    frames again, as a device tensor or as the list of host arrays by ``keep_on_device``.  Two renders of one photo need not agree to the
    byte (the networks run again in every call, and theirs is not a bit-exact route), so what a test wants to know of two calls -- that they
    ask for the same frames and treat them alike afterwards -- is asked on ONE set of frames: a call that passes other settings, another
    size or another photo misses the memory, renders for itself, and shows in ``rendered``."""

    def __init__(self, real):
        self.real, self.kept, self.rendered, self.calls, self.on_device = real, {}, [], [], []

    def __call__(self, settings, oc, module, keep_on_device=False, **kw):
        key = (oc['tensorRawImage'].cpu().numpy().tobytes(), repr(sorted((k, repr(v)) for k, v in settings.items())), repr(sorted((k, repr(v)) for k, v in kw.items())))
        self.calls.append(key)
        self.on_device.append(bool(keep_on_device))
        if key not in self.kept:
            self.kept[key] = self.real(settings, oc, module, keep_on_device=True, **kw).clone()
            self.rendered.append(key)
        frames = self.kept[key]
        if keep_on_device:
            return frames.clone()
        host = frames.cpu().numpy()
        return [host[i] for i in range(host.shape[0])]


def test_the_layers_of_a_pipeline_and_of_a_slideshow(OV, tmp_path, monkeypatch):
    """One Pipeline (seeded weights, 6 steps, --write-frames) and two synthetic 64 x 48 photos, every clip rendered once (OneRenderPerClip).
    With a caption and a watermark the Pipeline asks for the frames it asks for without them, left in HBM, and returns the twin applied to
    them -- the caption first --; the PNG frames decode to them, the GIF and the y4m file are written; Pipeline.render returns the same.  A
    slideshow of the two photos with captions, T = 2 and a caption fade of 1 is the twin on Pipeline.render's clips, joined, with the
    watermark on every frame; its junction frames carry no caption.  A Pipeline call without the options writes the same bytes before and after."""
    from ken_burns_effect_amd import kbe, pipeline, slideshow, synthetic, transition, yuv
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    images = [synthetic.make_rgbd(48, 64, seed)[0] for seed in (12, 13)]
    zoom = kbe.windows_for(64, 48, slideshow.NO_WINDOW, False)
    logo = np.dstack([oc.frames_of(12, 7, 1, 77)[0], np.linspace(0, 255, 84).astype(np.uint8).reshape(7, 12)])
    Image.fromarray(np.ascontiguousarray(logo[:, :, [2, 1, 0, 3]]), 'RGBA').save(str(tmp_path / 'logo.png'))        # (the file holds R, G, B: the frames are B, G, R)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=6)
    once = OneRenderPerClip(pipeline.common.process_kenburns)
    monkeypatch.setattr(pipeline.common, 'process_kenburns', once)
    before = pipe(images[0], zoom, str(tmp_path / 'before'))
    plain = np.stack(before)
    assert len(once.rendered) == 1 and once.on_device == [False]

    # the Pipeline with both layers
    options = dict(overlay=str(tmp_path / 'logo.png'), overlay_at='top-right', overlay_opacity=0.75, caption='A view', caption_at='top-right', caption_size=8, overlay_margin=2)
    for name, value in options.items():
        setattr(pipe, name, value)
    pipe.gif = pipe.y4m = True
    got = np.stack(pipe(images[0], zoom, str(tmp_path / 'layers')))
    assert len(once.rendered) == 1 and once.calls[1] == once.calls[0] and once.on_device == [False, True]            # (the same frames, asked to stay in HBM)
    text = OV.caption_image('A view', 8)
    cx, cy = OV.place('top-right', 64, 48, text.shape[1], text.shape[0], 2)
    want = oc.twin_over(oc.twin_over(plain, text, cx, cy, 256), logo, 64 - 12 - 2, 2, 192)
    assert np.array_equal(got, want) and (want != plain).any(axis=3).mean() > 0.05
    assert not np.array_equal(want, oc.twin_over(oc.twin_over(plain, logo, 64 - 12 - 2, 2, 192), text, cx, cy, 256))            # (both at the top right: the order shows where they meet)
    files = _files(tmp_path / 'layers')
    assert sorted(files) == sorted(['3d_kbe.mp4', '3d_kbe.gif', '3d_kbe.y4m'] + ['frames/%d.png' % i for i in range(6)])
    for i in range(6):
        png = Image.open(str(tmp_path / 'layers' / 'frames' / ('%d.png' % i)))
        assert png.size == (64, 48) and np.array_equal(np.asarray(png.convert('RGB')), want[i][:, :, ::-1])
    gif = Image.open(str(tmp_path / 'layers' / '3d_kbe.gif'))
    assert gif.size == (64, 48) and gif.n_frames == 11                       # (a clip plays forth and back)
    header = yuv.y4m_header(64, 48, 25)
    assert files['3d_kbe.y4m'].startswith(header + b'FRAME\n') and len(files['3d_kbe.y4m']) == len(header) + 11 * (6 + yuv.frame_bytes(64, 48))
    pipe.gif = pipe.y4m = None
    assert np.array_equal(np.stack(pipe(images[0], zoom, None)), want) and not (tmp_path / 'None').exists()
    rendered = pipe.render(images[0], zoom)
    assert rendered.is_cuda and np.array_equal(rendered.cpu().numpy(), want) and once.calls[-1] == once.calls[0] and len(once.rendered) == 1
    # refused before a network runs: nothing more was asked of process_kenburns
    asked = len(once.calls)
    pipe.overlay_margin = 30
    with pytest.raises(ValueError, match=r"^--caption 'A view': it is \d+x\d+ and the frames are 64x48: with a margin of 30"):
        pipe(images[0], zoom, str(tmp_path / 'refused'))
    assert len(once.calls) == asked and not (tmp_path / 'refused').exists()
    for name in options:
        setattr(pipe, name, None)

    # a slideshow: captions on their clips, the watermark on the joined frames
    clips = [pipe.render(image, zoom).cpu().numpy() for image in images]
    assert np.array_equal(clips[0], plain) and len(once.rendered) == 2
    request = OV.layers_request(overlay=str(tmp_path / 'logo.png'), overlay_at='top-right', overlay_opacity=0.75, caption='x', caption_size=8, overlay_margin=2)
    pipe.caption = 'not the show\'s'                                         # (the slideshow renders its clips without the Pipeline's own layers)
    held = dict(vars(pipe))
    show = slideshow.make(images, str(tmp_path / 'show'), pipe, 'dissolve', 2, captions=['First', 'Second\nphoto'], caption_fade=1, layers=request, gif=True, y4m=True)
    assert dict(vars(pipe)) == held                                          # (... and leaves the Pipeline as it found it: no attribute set, none changed)
    pipe.caption = None
    assert len(once.rendered) == 2 and once.calls[-2:] == [once.calls[0], once.calls[-3]]
    titled = []
    for clip, words, window in zip(clips, ('First', 'Second\nphoto'), ((0, 4), (2, 6))):
        title = OV.caption_image(words, 8)
        tx, ty = OV.place('bottom', 64, 48, title.shape[1], title.shape[0], 2)
        table = OV.opacity_table(6, window[0], window[1], 1)
        titled.append(oc.twin_over(clip, title, tx, ty, table))
        assert [(titled[-1][j] != clip[j]).any() for j in range(6)] == [v > 0 for v in table]
    assert OV.opacity_table(6, 0, 4, 1) == [128, 256, 256, 128, 0, 0] and OV.opacity_table(6, 2, 6, 1) == [0, 0, 128, 256, 256, 128]
    table = transition.progress_table(2)
    joined = np.stack([titled[0][i] for i in range(4)] + [tc.twin_blend(titled[0][4 + j][None], titled[1][j][None], 'dissolve', [table[j]])[0] for j in range(2)] + [titled[1][i] for i in range(2, 6)])
    want = oc.twin_over(joined, logo, 64 - 12 - 2, 2, 192)
    assert len(show) == 10 and np.array_equal(np.stack(show), want)
    # the junction's frames carry no caption: they are the blend of the clips' own frames, under the watermark alone
    for j in range(2):
        bare = tc.twin_blend(clips[0][4 + j][None], clips[1][j][None], 'dissolve', [table[j]])
        assert np.array_equal(show[4 + j], oc.twin_over(bare, logo, 64 - 12 - 2, 2, 192)[0])
    assert all((show[i] != oc.twin_over((clips[0][i] if i < 4 else clips[1][i - 4])[None], logo, 50, 2, 192)[0]).any() for i in (0, 1, 2, 3, 6, 7, 8, 9))
    files = _files(tmp_path / 'show')
    assert sorted(files) == sorted(['slideshow.mp4', 'slideshow.gif', 'slideshow.y4m'] + ['frames/%d.png' % i for i in range(10)])
    for i, frame in enumerate(show):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'show' / 'frames' / ('%d.png' % i))).convert('RGB')), frame[:, :, ::-1])
    with pytest.raises(ValueError, match=r'^--caption-fade 3: 0\.\.2, half of the 4 frames'):
        slideshow.make(images, str(tmp_path / 'refused'), pipe, 'dissolve', 2, captions=['a', 'b'], caption_fade=3)
    with pytest.raises(ValueError, match=r'^--caption: 1 captions for 2 photos'):
        slideshow.make(images, str(tmp_path / 'refused'), pipe, 'dissolve', 2, captions=['a'])
    assert not (tmp_path / 'refused').exists() and len(once.rendered) == 2

    # without the options: the same bytes as before
    pipe(images[0], zoom, str(tmp_path / 'after'))
    assert once.calls[-1] == once.calls[0] and once.on_device[-1] is False and len(once.rendered) == 2
    assert _files(tmp_path / 'after') == _files(tmp_path / 'before') and sorted(_files(tmp_path / 'before')) == ['3d_kbe.mp4'] + ['frames/%d.png' % i for i in range(6)]
