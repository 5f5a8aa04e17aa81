"""The colour grade on the GPU (include/kbe_grade.h; kernel: csrc/kbe_grade.hip): kbe_grade_u8 byte for byte against the NumPy twin
(tests/grade_cases.py) under guard bands and both poisons, the whole of every frame and its padding compared -- the entry works in place --,
at the shapes where the kernel can go wrong: every table size class, every cell edge and tie, every alignment class of a row, rows around
a lane's run and a wave's span, more items than the grid holds, the cut into launches; every refusal, a side stream, and the host side
built on it (grade.apply, Pipeline's grade under its layers, a slideshow of graded clips)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import grade_cases as gc
import grade_gpu as gg
import overlay_cases as oc
import stream_gpu
import transition_cases as tc
from test_overlay_gpu import OneRenderPerClip, _files

pytestmark = pytest.mark.gpu
run, assert_grade = gg.run_grade, gg.assert_grade


@pytest.fixture(scope='module')
def GR():
    from ken_burns_effect_amd import grade
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    grade.load()
    return grade


# -- the entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['random', 'rotation'])
@pytest.mark.parametrize('N', gc.SIZES)
@pytest.mark.parametrize('frame', gc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(GR, frame, N, kind):
    """37x50, 64x48 and 160x128 frames through tables of 2, 3, 17 and 33 nodes per axis -- noise, and the rotation of the channels, which a
    mistake in the order of the axes turns into another permutation --; two frames in one call at the strengths 256 and 150; rows padded by 4."""
    W, H = frame
    frames, table = gc.frames_of(W, H), gc.TABLES[kind](N)
    want = gc.twin_of(W, H, N, kind)
    assert (want != frames).any(axis=3).mean() > 0.5
    if kind == 'rotation' and N in gc.EXACT_SIZES:
        assert np.array_equal(want[0], frames[0][:, :, [1, 2, 0]])
    assert_grade(GR, frames, table, gc.STRENGTH, want, pad=4)


@pytest.mark.parametrize('N', [17, 33])
def test_every_cell_edge_clamp_and_tie(GR, N):
    """A 512x512 frame whose pixels are all 64^3 combinations of 64 byte values per channel -- 0, 255, the nodes' values at N = 17 and 33
    and their neighbours --: every cell edge, v = 255's clamp, every order of the fractions and every tie between them."""
    frame = gc.all_cells_frame()
    i, f = gc.cells(frame, N)
    assert frame.shape == (1, 512, 512, 3) and len(np.unique(frame.reshape(-1, 3), axis=0)) == 64 ** 3
    assert set(np.unique(i).tolist()) == set(range(N - 1)) and {0, 255} <= set(np.unique(f).tolist())
    orders = {tuple(o) for o in np.unique(np.argsort(-f.reshape(-1, 3), axis=1, kind='stable'), axis=0).tolist()}
    assert len(orders) == 6 and ((f[..., 0] == f[..., 1]) & (f[..., 1] == f[..., 2])).any() and ((f[..., 0] == f[..., 1]) & (f[..., 1] != f[..., 2])).any()
    assert_grade(GR, frame, gc.random(N), 256, None, poisons=(0xFF,))
    assert_grade(GR, frame, gc.rotation(N), 201, None, poisons=(0x00,), pad=1)


@pytest.mark.parametrize('shift', range(16))
def test_every_alignment_class(GR, shift):
    """40 x 20 frames whose rows lie 121 bytes apart, an odd number, so that a frame's rows walk through all sixteen classes of their
    address, the frame `shift` bytes off its allocation: two whole runs and one of 8 pixels per row, at every class, in sixteen calls."""
    W, H = 40, 20
    assert len({(shift + (3 * W + 1) * y) % 16 for y in range(H)}) == 16 and W % gg.RUN_PIXELS == 8
    assert_grade(GR, gc.frames_of(W, H), gc.random(17), (256, 99), None, pad=1, shift=shift, aligned=True)


@pytest.mark.parametrize('W', [gg.RUN_PIXELS - 1, gg.RUN_PIXELS, gg.RUN_PIXELS + 1, gg.SPAN_PIXELS - 1, gg.SPAN_PIXELS, gg.SPAN_PIXELS + 1])
def test_rows_around_a_lanes_run_and_a_waves_span(GR, W):
    """A lane owns 16 whole pixels and a wave takes 1024 pixels of a row: rows one pixel short of either, exact, and one pixel beyond (a
    row's bytes are whole pixels), the beyond being a run of one pixel and a second item with one lane at work.  At an address that is a
    multiple of 16, of 4 and odd; 5 rows, so that the items of a row's second span lie between the others'."""
    assert gg.RUN_PIXELS == 16 and gg.SPAN_PIXELS == 1024
    frames = gc.frames_of(W, 5, 1)
    want = gc.twin_grade(frames, gc.random(17), 256)
    for pad, shift in ((0, 0), (1, 4), (2, 7)):
        assert_grade(GR, frames, gc.random(17), 256, want, poisons=(0xFF,), pad=pad, shift=shift, aligned=True)


@pytest.mark.parametrize('N', gg.CLASS_SIZES)
def test_items_around_a_workgroups_share_and_beyond_the_grid(GR, N):
    """A workgroup takes one item per wave and trip -- 4, 4, 8 and 16 waves at the four LDS sizes --: frames of 17 pixels' width whose rows
    are one short of a workgroup's waves, exact, and one beyond; and a frame of 5 x 8200, more items than the largest grid holds (256 CUs x
    8 workgroups x 4 waves = 8192; 4096 at the two larger sizes), so that workgroups take a second trip and the last trip is not full."""
    waves = gg.GROUP_WAVES[N]
    table = gc.random(N)
    for H in (waves - 1, waves, waves + 1):
        assert_grade(GR, gc.frames_of(17, H, 1), table, 256, None, poisons=(0xFF,), pad=3)
    tall = gc.frames_of(5, 8200, 1)
    assert_grade(GR, tall, table, 256, None, poisons=(0x00,), pad=1)


@pytest.mark.parametrize('frame', [(1, 7), (1366, 3)], ids=lambda v: '%dx%d' % v)
def test_narrow_and_wide_frames(GR, frame):
    """W = 1: rows of three bytes, one lane per row.  1366 x 3: rows of 4098 bytes, a second span of 342 pixels whose last run has 6."""
    W, H = frame
    frames = gc.frames_of(W, H)
    for kw in (dict(), dict(pad=3, shift=13)):
        want = assert_grade(GR, frames, gc.random(33), (256, 77), None, **kw)
        assert (want != frames).any()


def test_the_cut_into_launches(GR):
    """A launch carries 12 frames: 13 frames with 13 strengths are 12 + 1, every frame changed in its own way.  Frames at strength 0 are in
    no launch and stay untouched: 12 of those and 13 that are graded make 25 frames in two launches."""
    W, H, n = 40, 16, GR.FRAMES_PER_LAUNCH + 1
    assert n == 13
    frames, table = gc.frames_of(W, H, n), gc.random(17)
    strengths = [40 + 18 * i for i in range(n)]
    want = gc.twin_grade(frames, table, strengths)
    rotated = gc.twin_grade(frames, table, strengths[1:] + strengths[:1])
    assert all(not np.array_equal(want[i], frames[i]) and not np.array_equal(rotated[i], want[i]) for i in range(n))
    assert_grade(GR, frames, table, strengths, want, pad=1)
    more = gc.frames_of(W, H, 25)
    strengths = [0 if i % 2 == 0 and i < 24 else 200 for i in range(25)]
    want = assert_grade(GR, more, table, strengths, None, poisons=(0xFF,))
    assert [np.array_equal(want[i], more[i]) for i in range(25)] == [s == 0 for s in strengths] and strengths.count(0) == 12


def test_the_extremes(GR):
    """Strength 0: the frames as they were.  An exact identity table at strength 256: the frames as they were.  A constant table: that colour
    everywhere.  Strength 1 and 255 on all-0 and all-255 frames."""
    W, H = 37, 12
    frames = gc.frames_of(W, H, 3)
    assert_grade(GR, frames, gc.random(17), 0, frames, pad=1)
    for N in gc.EXACT_SIZES:
        assert_grade(GR, frames, gc.identity(N), 256, frames, poisons=(0xFF,), shift=1)
    want = assert_grade(GR, frames, gc.constant(33), 256, None, pad=1)
    assert (want == (17, 200, 99)).all()
    want = assert_grade(GR, frames, gc.constant(2), (0, 256, 128), None)
    assert np.array_equal(want[0], frames[0]) and (want[1] == (17, 200, 99)).all() and not np.array_equal(want[2], frames[2])
    white, black = np.full((2, H, W, 3), 255, np.uint8), np.zeros((2, H, W, 3), np.uint8)
    for frames_, colour in ((white, (0, 0, 0)), (black, (255, 255, 255)), (white, (255, 255, 255)), (black, (0, 0, 0))):
        want = assert_grade(GR, frames_, gc.constant(3, colour), (1, 255), None, poisons=(0x00,), pad=2)
        c, g = int(frames_[0, 0, 0, 0]), colour[0]
        assert [int(want[k, 0, 0, 0]) for k in (0, 1)] == [(c * 255 + g + 128) >> 8, (c + g * 255 + 128) >> 8]


def _frame_bytes(a):
    return (a['H'] - 1) * a['stride_bytes'] + 3 * a['W']


OVERLAPS_FRAME, OVERLAPS_TABLE = 'an element of frames_u8 overlaps another frame', 'an element of frames_u8 overlaps the table'
REFUSALS = {'null frames': (lambda a: a.update(frames_u8=None), 'null frames_u8'), 'null lut': (lambda a: a.update(lut=None), 'null lut'),
            'null strength': (lambda a: a.update(strength=None), 'null strength'), 'n = 0': (lambda a: a.update(n=0), 'n < 1'), 'n = -1': (lambda a: a.update(n=-1), 'n < 1'),
            'W = 65536': (lambda a: a.update(W=65536, stride_bytes=3 * 65536), 'W or H outside 1..65535'), 'W = 0': (lambda a: a.update(W=0), 'W or H outside 1..65535'),
            'H = 0': (lambda a: a.update(H=0), 'W or H outside 1..65535'), 'H = 65536': (lambda a: a.update(H=65536), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'N = 1': (lambda a: a.update(N=1), 'N outside 2..33'), 'N = 34': (lambda a: a.update(N=34), 'N outside 2..33'),
            'a misaligned table': (lambda a: a.update(lut=a['lut'] + 2), 'lut is not 4-byte aligned'),
            'null frame 1': (lambda a: a['frames_u8'].__setitem__(1, None), 'null element of frames_u8'),
            'strength 257': (lambda a: a['strength'].__setitem__(1, 257), 'an element of strength outside 0..256'),
            'strength -1': (lambda a: a['strength'].__setitem__(0, -1), 'an element of strength outside 0..256'),
            'the same frame twice': (lambda a: a['frames_u8'].__setitem__(1, a['frames_u8'][0]), OVERLAPS_FRAME),
            'one byte of the other frame': (lambda a: a['frames_u8'].__setitem__(0, a['frames_u8'][1] - _frame_bytes(a) + 1), OVERLAPS_FRAME),
            'the table is a frame': (lambda a: a.update(lut=a['frames_u8'][1]), OVERLAPS_TABLE),
            'the table on a frames last byte': (lambda a: a.update(lut=(a['frames_u8'][0] + _frame_bytes(a) - 1) & ~3), OVERLAPS_TABLE),
            'a frame on the tables last byte': (lambda a: a['frames_u8'].__setitem__(1, a['lut'] + 4 * a['N'] ** 3 - 1), OVERLAPS_TABLE)}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_frames_untouched(GR, what):
    from ken_burns_effect_amd import _native
    W, H = gc.FRAMES[0]
    change, text = REFUSALS[what]
    frames = gc.frames_of(W, H)
    rc, got = run(GR, frames, gc.random(17), gc.STRENGTH, pad=2, change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_grade_u8: ' + text
    assert np.array_equal(got[:, :, :3 * W].reshape(2, H, W, 3), frames) and (got[:, :, 3 * W:] == 0xFF).all()


def test_frames_that_touch_are_taken(GR):
    """Frames back to back in one tensor -- the next begins with the byte behind the last -- are no overlap; the table in its three forms."""
    host, table = gc.frames_of(37, 50, 3), gc.random(17)
    want = gc.twin_grade(host, table, (256, 100, 3))
    for form in (torch.from_numpy(table.copy()), torch.from_numpy(gc.packed(table).view(np.int32).copy())):
        frames = torch.from_numpy(host.copy()).cuda()
        got = GR.apply(frames, form.cuda(), (256, 100, 3))
        assert got is frames and np.array_equal(got.cpu().numpy(), want)


def _pointers(t):
    return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])


def test_on_a_side_stream_behind_a_delay(GR):
    """The entry called raw with the handle of a non-blocking side stream behind stream_gpu's delay: it returns while the delay runs, and the
    result is the twin, bit for bit; the frames and the table hold a decoy until the delay has run out."""
    from ken_burns_effect_amd import _native
    n, H, W, N = 13, 37, 50, 33
    right = [torch.from_numpy(gc.frames_of(W, H, n).copy()).cuda(), torch.from_numpy(gc.random(N).copy()).cuda()]
    decoy = [torch.from_numpy(gc.frames_of(W, H, n, 150).copy()).cuda(), torch.from_numpy(gc.random(N, 9).copy()).cuda()]
    frames, table = [t.clone() for t in decoy]
    strengths = [256 - 9 * i for i in range(n)]

    def call():
        GR._call('kbe_grade_u8', _pointers(frames), n, W, H, 3 * W, table.data_ptr(), N, (ctypes.c_int32 * n)(*strengths), _native._stream())
        return frames
    what = 'grade_u8'
    got, want = stream_gpu.hold(what, 'bits', [frames, table], right, decoy, call)
    assert what in stream_gpu.ENQUEUED                                      # (the entry had returned while the delay still ran)
    assert np.array_equal(got[0], gc.twin_grade(right[0].cpu().numpy(), right[1].cpu().numpy(), strengths)) and np.array_equal(got[0], want[0])


# -- the module ----------------------------------------------------------------------------------
def test_apply_and_its_refusals(GR):
    from ken_burns_effect_amd import _native
    W, H = gc.FRAMES[2]
    n = 13
    host, table = gc.frames_of(W, H, n), gc.sepia()
    frames, lut = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(table.copy()).cuda()
    got = GR.apply(frames, lut)
    assert got is frames and np.array_equal(got.cpu().numpy(), gc.twin_grade(host, table, 256))
    frames.copy_(torch.from_numpy(host.copy()))
    strengths = [20 * i for i in range(n)]
    assert np.array_equal(GR.apply(frames, lut, strengths).cpu().numpy(), gc.twin_grade(host, table, strengths))
    before = frames.clone()
    for args in ((frames.cpu(), lut), (frames, lut.cpu()), (frames.int(), lut), (frames[0], lut), (frames[:, :, ::2], lut), (frames, lut[..., :3]), (frames, lut[None]),
                 (frames, lut.float()), (frames, lut[:, ::2]), (frames, lut[:32]), (frames, None), (None, lut), (frames, lut[:1, :1, :1]), (frames, lut, [256] * 12), (frames, lut, 0.5),
                 (frames, lut, 257), (frames, lut, -1), (frames, lut, None), (frames, lut, 'all'), (frames, frames[0].view(-1)[:4 * 17 ** 3].view(17, 17, 17, 4))):
        with pytest.raises(_native.KbeError, match=r'grade\.apply|kbe_grade_u8: an element of frames_u8 overlaps the table'):
            GR.apply(*args)
    assert torch.equal(frames, before)


# -- the routes ----------------------------------------------------------------------------------
ENV = ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES', 'KBE_Y4M',
       'KBE_OVERLAY', 'KBE_OVERLAY_AT', 'KBE_OVERLAY_OPACITY', 'KBE_CAPTION', 'KBE_CAPTION_AT', 'KBE_CAPTION_SIZE', 'KBE_LUT', 'KBE_GRADE', 'KBE_LOOK', 'KBE_LUT_STRENGTH')


def test_the_grade_of_a_pipeline_and_of_a_slideshow(GR, tmp_path, monkeypatch):
    """One Pipeline (seeded weights, 6 steps, --write-frames) and two synthetic 64 x 48 photos, every clip rendered once (OneRenderPerClip).
    With look='sepia', lut_strength=0.75 and a caption the Pipeline asks for the frames it asks for without them, left in HBM, and returns
    the caption's twin on the grade's twin of them; the caption's own pixels are not graded; the PNG frames decode to those frames, the GIF
    and the y4m file are written; Pipeline.render returns the same.  A slideshow of the two photos with T = 2 is the join of the graded
    clips.  A Pipeline call without the options writes the same bytes before and after."""
    from ken_burns_effect_amd import kbe, overlay, pipeline, slideshow, synthetic, transition, yuv
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

    # the Pipeline with a grade under a caption
    table = gc.sepia(True)
    assert np.array_equal(gc.packed(table), GR.grade_for(GR.grade_request(look='sepia'))[0])
    pipe.look, pipe.lut_strength, pipe.caption, pipe.caption_at, pipe.caption_size, pipe.overlay_margin = 'sepia', 0.75, 'A view', 'top-right', 8, 2
    pipe.gif = pipe.y4m = True
    got = np.stack(pipe(images[0], zoom, str(tmp_path / 'graded')))
    assert len(once.rendered) == 1 and once.calls[1] == once.calls[0] and once.on_device == [False, True]            # (the same frames, asked to stay in HBM)
    text = overlay.caption_image('A view', 8)
    cx, cy = overlay.place('top-right', 64, 48, text.shape[1], text.shape[0], 2)
    graded = gc.twin_grade(plain, table, 192)
    want = oc.twin_over(graded, text, cx, cy, 256)
    assert np.array_equal(got, want) and (graded != plain).any(axis=3).mean() > 0.5
    assert not np.array_equal(want, gc.twin_grade(oc.twin_over(plain, text, cx, cy, 256), table, 192))                 # (the caption is not graded)
    # (where the caption is most opaque, alpha a, a frame's pixel lies within 255 - a (+ 1 of rounding) of the caption's own colour, whatever the grade made of the frame)
    most = int(text[:, :, 3].max())
    solid = text[:, :, 3] == most
    assert most > 128 and all((np.abs(got[i, cy:cy + text.shape[0], cx:cx + text.shape[1]][solid].astype(int) - text[:, :, :3][solid]) <= 255 - most + 1).all() for i in range(6))
    files = _files(tmp_path / 'graded')
    assert sorted(files) == sorted(['3d_kbe.mp4', '3d_kbe.gif', '3d_kbe.y4m'] + ['frames/%d.png' % i for i in range(6)])
    for i in range(6):
        png = Image.open(str(tmp_path / 'graded' / 'frames' / ('%d.png' % i)))
        assert png.size == (64, 48) and np.array_equal(np.asarray(png.convert('RGB')), want[i][:, :, ::-1])
    gif = Image.open(str(tmp_path / 'graded' / '3d_kbe.gif'))
    assert gif.size == (64, 48) and gif.n_frames == 11
    header = yuv.y4m_header(64, 48, 25)
    assert files['3d_kbe.y4m'].startswith(header + b'FRAME\n') and len(files['3d_kbe.y4m']) == len(header) + 11 * (6 + yuv.frame_bytes(64, 48))
    pipe.gif = pipe.y4m = None
    assert np.array_equal(np.stack(pipe(images[0], zoom, None)), want) and not (tmp_path / 'None').exists()
    rendered = pipe.render(images[0], zoom)
    assert rendered.is_cuda and np.array_equal(rendered.cpu().numpy(), want) and once.calls[-1] == once.calls[0] and len(once.rendered) == 1
    # the grade alone: on_device as well, and R, G, B frames take the table in their order
    pipe.caption = pipe.caption_at = pipe.caption_size = pipe.overlay_margin = None
    assert np.array_equal(np.stack(pipe(images[0], zoom, None)), graded) and once.on_device[-1] is True
    assert np.array_equal(np.stack(pipe(images[0], zoom, None, pretrained_estim=True)), gc.twin_grade(plain, gc.sepia(False), 192))
    assert not np.array_equal(gc.sepia(False), gc.sepia(True))
    # refused before a network runs: nothing more was asked of process_kenburns
    asked = len(once.calls)
    pipe.look = 'teal'
    with pytest.raises(ValueError, match=r'^--look teal: mono or sepia$'):
        pipe(images[0], zoom, str(tmp_path / 'refused'))
    with pytest.raises(ValueError, match=r'^--look teal: mono or sepia$'):
        pipe.render(images[0], zoom)
    assert len(once.calls) == asked and not (tmp_path / 'refused').exists()

    # a slideshow: the clips graded by Pipeline.render, the transition blends graded frames
    pipe.look, pipe.lut_strength = None, None
    clips = [pipe.render(image, zoom).cpu().numpy() for image in images]
    assert np.array_equal(clips[0], plain) and len(once.rendered) == 2
    pipe.look, pipe.grade = 'sepia', 'contrast=1.2,brightness=0.9'
    table = np.ascontiguousarray(GR.quantise(GR.bake(contrast=1.2, brightness=0.9, look='sepia'), True)).view(np.uint8).reshape(33, 33, 33, 4)
    show = slideshow.make(images, str(tmp_path / 'show'), pipe, 'dissolve', 2)
    assert len(once.rendered) == 2
    toned = [gc.twin_grade(clip, table, 256) for clip in clips]
    blend = transition.progress_table(2)
    joined = np.stack([toned[0][i] for i in range(4)] + [tc.twin_blend(toned[0][4 + j][None], toned[1][j][None], 'dissolve', [blend[j]])[0] for j in range(2)] + [toned[1][i] for i in range(2, 6)])
    assert len(show) == 10 and np.array_equal(np.stack(show), joined) and not np.array_equal(toned[0], clips[0])
    for i, frame in enumerate(show):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'show' / 'frames' / ('%d.png' % i))).convert('RGB')), frame[:, :, ::-1])
    pipe.lut_strength = 2
    with pytest.raises(ValueError, match=r'^--lut-strength 2: above 0 and at most 1$'):
        slideshow.make(images, str(tmp_path / 'refused'), pipe, 'dissolve', 2)
    assert not (tmp_path / 'refused').exists() and len(once.rendered) == 2
    pipe.look = pipe.grade = pipe.lut_strength = None

    # without the options: the same bytes as before
    pipe(images[0], zoom, str(tmp_path / 'after'))
    assert once.calls[-1] == once.calls[0] and once.on_device[-1] is False and len(once.rendered) == 2
    assert _files(tmp_path / 'after') == _files(tmp_path / 'before') and sorted(_files(tmp_path / 'before')) == ['3d_kbe.mp4'] + ['frames/%d.png' % i for i in range(6)]
