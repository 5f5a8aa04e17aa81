"""The exact area-average reduction on the GPU (include/kbe_area.h; kernel: csrc/kbe_area.hip): kbe_area_reduce_u8 byte for byte against the
NumPy twin (tests/area_cases.py) under guard bands, padded strides, an unaligned output and argument checks, and the host side built on it
(area.reduce, gif.write_gif(size=, every=), Pipeline under KBE_GIF_WIDTH)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import area_cases as ac
import encoder_gpu as eg
import filter_gpu as fg
import gif_cases as gc
from guarded import SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    from ken_burns_effect_amd import area
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    area.load()
    return area


@pytest.fixture(scope='module')
def rendered():
    return eg.rendered(eg.kernels())


stream, run = fg.stream, fg.run_area                  # (the raw call on guarded buffers: tests/filter_gpu.py)


def assert_reduced(A, frames, w, h, want, **kw):
    rc, got = run(A, frames, w, h, **kw)
    assert rc == 0
    n = len(got)
    assert np.array_equal(got[:, :, :3 * w].reshape(n, h, w, 3), want)
    assert (got[:, :, 3 * w:] == SENTINEL).all()                       # the rows' padding is not written


@pytest.mark.parametrize('name', sorted(ac.TARGETS))
def test_the_device_is_the_twin_byte_for_byte(A, name):
    """160x128 -> a non-integer ratio, an integer factor, a ratio just under 1, a copy, one pixel; 3 frames."""
    w, h = ac.TARGETS[name]
    assert_reduced(A, ac.photo(3), w, h, ac.twin_of(name, 3))


def test_smaller_than_a_tile(A):
    assert_reduced(A, ac.small(), 3, 5, ac.twin_reduce(ac.small(), 3, 5))


def test_thirteen_frames_take_two_launches(A):
    assert_reduced(A, ac.photo(13), 75, 60, ac.twin_of('non_integer', 13))


def test_several_tiles_and_strips_on_both_axes(A):
    """1000x1000 -> 333x777: six tiles across and 195 down, a ratio above 3 across (a tile's span there is 193 sources, at the tile's
    full width), and the last tile of each axis short."""
    frame, want = ac.large()
    assert_reduced(A, frame, 333, 777, want)


def test_a_span_wider_than_a_strip(A):
    """1000x40 -> 64x3: one tile whose 64 columns span all 1000 sources -- three strips of 340 across -- and whose 3 rows span 40, three
    strips of 16 down."""
    frame = ac.large()[0][:, :40]
    assert_reduced(A, frame, 64, 3, ac.twin_reduce(frame, 64, 3))


@pytest.mark.parametrize('name', ['non_integer', 'just_under_1', 'copy'])
def test_padded_strides_and_an_unaligned_output(A, name):
    """Source rows 7 bytes apart beyond their pixels (every row at another alignment), output rows 5, the output 3 bytes off its allocation:
    the twin's bytes, the padding of every row and the bands around every frame untouched."""
    w, h = ac.TARGETS[name]
    assert_reduced(A, ac.photo(2), w, h, ac.twin_of(name, 3)[:2], pad=7, out_pad=5, shift=3)
    assert_reduced(A, ac.photo(2), w, h, ac.twin_of(name, 3)[:2], pad=1, out_pad=0, shift=1)


REFUSALS = {'null frames': lambda a: a.update(frames_u8=None),
            'null out': lambda a: a.update(out_u8=None),
            'null frame 1': lambda a: a['frames_u8'].__setitem__(1, None),
            'null output 1': lambda a: a['out_u8'].__setitem__(1, None),
            'n = 0': lambda a: a.update(n_frames=0),
            'W = 0': lambda a: a.update(W=0),
            'H = 0': lambda a: a.update(H=0),
            'W = 65536': lambda a: a.update(W=65536, stride_bytes=3 * 65536),
            'H = 65536': lambda a: a.update(H=65536),
            'w > W': lambda a: a.update(w=a['W'] + 1, out_stride_bytes=3 * (a['W'] + 1)),
            'h > H': lambda a: a.update(h=a['H'] + 1),
            'w = 0': lambda a: a.update(w=0),
            'h = 0': lambda a: a.update(h=0),
            'w = -1': lambda a: a.update(w=-1),
            'stride < 3 W': lambda a: a.update(stride_bytes=3 * a['W'] - 1),
            'out stride < 3 w': lambda a: a.update(out_stride_bytes=3 * a['w'] - 1)}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(A, what):
    from ken_burns_effect_amd import _native
    rc, got = run(A, ac.small(), 3, 5, change=REFUSALS[what])
    assert rc == -1 and _native.load().kbe_last_error().decode().startswith('kbe_area_reduce_u8: ')
    assert (got == SENTINEL).all()


def test_area_reduce_and_its_refusals(A):
    from ken_burns_effect_amd import _native
    frames = torch.from_numpy(np.array(ac.photo(13))).cuda()
    got = A.reduce(frames, 75, 60)
    assert got.shape == (13, 60, 75, 3) and got.dtype == torch.uint8 and got.device == frames.device
    assert np.array_equal(got.cpu().numpy(), ac.twin_of('non_integer', 13))
    for w, h in ((161, 128), (160, 129), (0, 5), (5, 0)):
        with pytest.raises(_native.KbeError, match='only reduced'):
            A.reduce(frames, w, h)
    with pytest.raises(_native.KbeError):
        A.reduce(frames.cpu(), 75, 60)


def _decoded(path):
    im = Image.open(path)
    frames = []
    for i in range(im.n_frames):
        im.seek(i)
        frames.append(np.asarray(im.convert('RGB')))
    return im, frames


def _expected(raw, palette, bgr, dither):
    return palette[gc.lut_of(palette)[gc.cells(raw, bgr, dither)]]


def test_write_gif_at_a_size_and_a_rate(A, tmp_path):
    """13 photo-like frames, size=(64, 48), every=2: frames 0, 2 .. 12 forth and back at 12.5 a second, each the twin's reduction of its frame."""
    from ken_burns_effect_amd import gif
    raw = ac.photo(13)
    in_hbm = torch.from_numpy(np.array(raw)).cuda()
    path = str(tmp_path / 'small.gif')
    palette, count = gif.write_gif(path, in_hbm, fps=25, bgr=True, size=(64, 48), every=2)
    kept = [0, 2, 4, 6, 8, 10, 12]
    order = kept + kept[-2::-1]
    im, frames = _decoded(path)
    assert count == im.n_frames == len(frames) == len(order) == 13 and im.size == (64, 48) and im.info['loop'] == 0 and im.info['duration'] == 10 * gif.delay_for(12.5) == 80
    small = ac.twin_reduce(raw, 64, 48)
    assert np.array_equal(palette, gif.palette_from_histogram(gc.hist_of(small[kept], True)))
    for i, frame in zip(order, frames):
        assert np.array_equal(frame, _expected(small[i], palette, True, gc.DITHER)), i
    # a step that does not divide: the last frame is kept all the same
    _, count = gif.write_gif(path, in_hbm, fps=25, bgr=True, size=(64, 48), every=5)
    im, frames = _decoded(path)
    assert count == im.n_frames == 7 and im.info['duration'] == 10 * gif.delay_for(5.0) == 200
    palette = gc.read_gif(open(path, 'rb').read())['palette']
    for i, frame in zip([0, 5, 10, 12, 10, 5, 0], frames):
        assert np.array_equal(frame, _expected(small[i], palette, True, gc.DITHER)), i


def test_write_gif_on_the_rendered_scene(A, rendered, tmp_path):
    """The issue's case: write_gif(..., size=(64, 48), every=2) on the rendered scene's two frames; and without the two arguments the file is
    the one write_gif writes without knowing them."""
    from ken_burns_effect_amd import gif
    in_hbm, raw = rendered
    path, plain, again = (str(tmp_path / name) for name in ('small.gif', 'plain.gif', 'again.gif'))
    palette, count = gif.write_gif(path, in_hbm, fps=25, bgr=True, size=(64, 48), every=2)
    kept = gif.kept_frames(len(raw), 2)
    order = kept + kept[-2::-1]
    im, frames = _decoded(path)
    assert kept == [0, 1] and count == im.n_frames == len(frames) == len(order) and im.size == (64, 48) and im.info['duration'] == 10 * gif.delay_for(12.5)
    small = ac.twin_reduce(np.stack(raw), 64, 48)
    for i, frame in zip(order, frames):
        assert np.array_equal(frame, _expected(small[i], palette, True, gc.DITHER)), i
    gif.write_gif(plain, in_hbm, fps=25, bgr=True)
    gif.write_gif(again, in_hbm, fps=25, bgr=True, size=None, every=1)
    data = open(plain, 'rb').read()
    assert data == open(again, 'rb').read()
    im, frames = _decoded(io.BytesIO(data))
    assert im.size == (128, 96) and im.n_frames == 3 and im.info['duration'] == 40


def _stub(P, output_frames):
    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = output_frames, False, 2, {}, None, torch.device('cuda:0')

        def estimate(self, tensorImage):
            return self.objectCommon
    return Stub()


def test_the_pipeline_writes_a_narrower_gif_and_nothing_else_changes(A, rendered, monkeypatch, tmp_path):
    """Pipeline._run with KBE_GIF=1 KBE_GIF_WIDTH=64: 3d_kbe.gif is 64 wide (and 48 high: the aspect ratio), every other file is byte for
    byte the run's without the width; a width above the image's is refused before anything is rendered."""
    from ken_burns_effect_amd import pipeline as P
    in_hbm, raw = rendered
    asked = []

    def kenburns(settings, oc, module, keep_on_device=False):
        asked.append(keep_on_device)
        return in_hbm if keep_on_device else [f for f in raw]
    monkeypatch.setattr(P.common, 'process_kenburns', kenburns)
    monkeypatch.setattr(P.shutil, 'which', lambda name: None)
    for name in ('KBE_GIF_DITHER', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('KBE_GIF', '1')
    monkeypatch.setenv('KBE_PNG', 'native')
    monkeypatch.setenv('KBE_JPEG', 'native')
    image, zoom = torch.zeros(1, 3, 96, 128), {'objectFrom': {}, 'objectTo': {}}

    def files_of(directory):
        return {str(p.relative_to(directory)): p.read_bytes() for p in sorted(directory.rglob('*')) if p.is_file()}
    _stub(P, True)(image, zoom, str(tmp_path / 'full'))
    monkeypatch.setenv('KBE_GIF_WIDTH', '64')
    _stub(P, True)(image, zoom, str(tmp_path / 'narrow'))
    full, narrow = files_of(tmp_path / 'full'), files_of(tmp_path / 'narrow')
    before, after = full.pop('3d_kbe.gif'), narrow.pop('3d_kbe.gif')
    assert narrow == full and '3d_kbe.mp4' in full and 'frames/1.png' in full
    assert Image.open(io.BytesIO(before)).size == (128, 96)
    im, frames = _decoded(io.BytesIO(after))
    assert im.size == (64, 48) and im.n_frames == 3 and im.info['duration'] == 40
    palette = gc.read_gif(after)['palette']
    small = ac.twin_reduce(np.stack(raw), 64, 48)
    for i, frame in zip((0, 1, 0), frames):
        assert np.array_equal(frame, _expected(small[i], palette, True, gc.DITHER))
    # the rate: every second frame of two is both of them, shown twice as long
    monkeypatch.setenv('KBE_GIF_FPS', '12.5')
    _stub(P, False)(image, zoom, str(tmp_path / 'slow'))
    im = Image.open(str(tmp_path / 'slow' / '3d_kbe.gif'))
    assert im.size == (64, 48) and im.n_frames == 3 and im.info['duration'] == 80
    monkeypatch.setenv('KBE_GIF_WIDTH', '129')
    calls = len(asked)
    with pytest.raises(ValueError, match='only ever reduced'):
        _stub(P, False)(image, zoom, str(tmp_path / 'wide'))
    assert len(asked) == calls
