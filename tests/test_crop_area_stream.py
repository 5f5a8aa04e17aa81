"""The crop + exact area-average reduction (include/kbe_crop_area.h) without a GPU: csrc/kbe_crop_area_block.h executed serially
(tests/crop_area_check.cpp) against a brute-force restatement, against the NumPy twin (tests/crop_area_cases.py) and, its patch, against the
suite's restatement of cv2.getRectSubPix (tests/opencv_8u_restatement.c); the twin's properties; the binding (crop_area.py) held to what
tests/test_header_bindings.py holds the two older headers to; the command line's --width and Pipeline(width=); and what the one-pass route
is worth beside reducing the frames written today."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest
from PIL import Image

import area_cases as ac
import crop_area_cases as cc
import gif_cases as gc
import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY_CROP = [(frame, name) for frame in cc.FRAMES for name in sorted(cc.OFF)]


# -- the definition ---------------------------------------------------------------------------
def test_the_header_against_brute_force():
    """crop_area_check.cpp builds, and csrc/kbe_crop_area_block.h run serially equals "patch, then sub-cell area sum" at every (W, cw, w) up
    to 6 per axis: 56 x 56 cases, all four parities of (W - cw, H - ch) among the crops."""
    m = re.search(r'brute: cases (\d+), pixels (\d+), mismatches (\d+), bad patches (\d+), bad weights (\d+), bad starts (\d+), parities (\d+) (\d+) (\d+) (\d+)', cc.ask('brute', 6))
    cases, pixels, mismatches, bad_patches, bad_weights, bad_starts, ee, eo, oe, oo = (int(v) for v in m.groups())
    assert cases == 56 * 56 and pixels == 126 * 126 and mismatches == 0 and bad_patches == 0 and bad_weights == 0 and bad_starts == 0
    assert (ee, eo, oe, oo) == (12 * 12, 12 * 9, 9 * 12, 9 * 9)           # (pairs cw <= W <= 6 with W - cw even: 12, odd: 9)


@pytest.mark.parametrize('frame, name', EVERY_CROP, ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_the_header_is_the_twin(frame, name):
    """crop_reduce_pixel of csrc/kbe_crop_area_block.h on the GPU suite's frames, rows padded: the NumPy twin byte for byte, at every target."""
    crop = cc.crop_of(frame, name)
    for size in cc.targets(crop).values():
        assert np.array_equal(cc.header_reduce(cc.frames(*frame), crop, size, pad=5), cc.twin_of(frame[0], frame[1], crop, size)), (crop, size)


def test_the_header_is_the_twin_across_strips():
    frame = cc.wide()
    assert np.array_equal(cc.header_reduce(frame, (690, 19), (345, 7)), cc.twin_reduce(frame, (690, 19), (345, 7)))
    tall = np.ascontiguousarray(frame.transpose(0, 2, 1, 3))
    assert np.array_equal(cc.header_reduce(tall, (19, 690), (7, 345)), cc.twin_reduce(tall, (19, 690), (7, 345)))


@pytest.fixture(scope='module')
def cvr(tmp_path_factory):
    """tests/opencv_8u_restatement.c as the suite builds it (tests/test_opencv_restatement.py); read, not edited."""
    so = str(tmp_path_factory.mktemp('cvr') / 'libcvr.so')
    subprocess.check_call(['gcc', '-O2', '-std=c99', '-fPIC', '-shared', '-ffp-contract=off', os.path.join(ROOT, 'tests', 'opencv_8u_restatement.c'), '-o', so, '-lm'])
    lib = ctypes.CDLL(so)
    lib.cvr_get_rect_sub_pix.restype = None
    lib.cvr_get_rect_sub_pix.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int, c_int, ctypes.c_float, ctypes.c_float]
    return lib


@pytest.mark.parametrize('frame, name', EVERY_CROP, ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_the_patch_is_get_rect_sub_pix(cvr, frame, name):
    """The header's patch and the twin's against the restatement of cv2.getRectSubPix(frame, (cw, ch), (W / 2, H / 2)): the four parities, and
    cw == W and ch == H, where the last taps lie beyond the frame and repeat its border."""
    W, H = frame
    cw, ch = cc.crop_of(frame, name)
    noise = np.ascontiguousarray(gc.noise(H, W, 3 + W))
    want = np.empty((ch, cw, 3), np.uint8)
    cvr.cvr_get_rect_sub_pix(noise.ctypes.data, W, H, want.ctypes.data, cw, ch, W / 2.0, H / 2.0)
    assert np.array_equal(cc.header_reduce(noise[None], (cw, ch), None, pad=2)[0], want)
    assert np.array_equal(cc.twin_patch(noise, cw, ch), want)


# -- properties of the twin --------------------------------------------------------------------
def test_a_constant_frame_stays_constant():
    for value in (0, 1, 137, 254, 255):
        for (W, H), name in ((cc.FRAMES[0], 'ee'), (cc.FRAMES[1], 'oe'), (cc.FRAMES[1], 'full'), (cc.FRAMES[2], 'eo')):
            crop = cc.crop_of((W, H), name)
            for size in cc.targets(crop).values():
                assert (cc.twin_reduce(np.full((H, W, 3), value, np.uint8), crop, size) == value).all()


@pytest.mark.parametrize('frame, name', EVERY_CROP, ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_the_crops_own_size_gives_the_patch_itself(frame, name):
    crop = cc.crop_of(frame, name)
    assert np.array_equal(cc.twin_reduce(cc.frames(*frame), crop, crop), cc.twin_patch(cc.frames(*frame), *crop))


@pytest.mark.parametrize('frame', cc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_a_crop_on_whole_pixels_is_the_area_reduction_of_the_sliced_rectangle(frame):
    """W - cw and H - ch odd: the patch is the raw rectangle at ((W - cw + 1) / 2, (H - ch + 1) / 2), and the route is area_cases' reduction of it."""
    W, H = frame
    cw, ch = cc.crop_of(frame, 'oo')
    x, y = (W - cw + 1) // 2, (H - ch + 1) // 2
    sliced = cc.frames(W, H)[:, y:y + ch, x:x + cw]
    for size in cc.targets((cw, ch)).values():
        assert np.array_equal(cc.twin_reduce(cc.frames(W, H), (cw, ch), size), ac.twin_reduce(sliced, *size))


def test_a_frames_bytes_do_not_depend_on_its_neighbours():
    W, H = cc.FRAMES[2]
    five = cc.frames(W, H, 5)
    crop = cc.crop_of((W, H), 'ee')
    size = cc.targets(crop)['under_2']
    together = cc.twin_reduce(five, crop, size)
    for i in (0, 2, 4):
        assert np.array_equal(cc.twin_reduce(five[i], crop, size), together[i])
        assert np.array_equal(cc.twin_reduce(five[[4 - i, i, 2]], crop, size)[1], together[i])
    assert np.array_equal(cc.header_reduce(five[[3, 1]], crop, size)[1], together[1])


# -- the binding -------------------------------------------------------------------------------
p, i, z = c_void_p, c_int, c_size_t
NULL_CALL = (None, 1, 4, 4, 12, 3, 3, None, 2, 2, 6, None)
CROP_AREA = thb.Binding(
    'crop_area', 'kbe_crop_area',
    # frames, n, W, H, stride; crop w, crop h; out, w, h, out stride; stream
    {'kbe_crop_area_abi_version': (c_int, []), 'kbe_crop_area_u8': (c_int, [p, i, i, i, i, i, i, p, i, i, i, p])},
    'kbe_crop_area_abi_version', ['#define KBE_CROP_AREA_ABI_VERSION 1\n'], ['KBE_CROP_AREA_BGR'], {'ABI_VERSION': 1},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n')],
    ('kbe_crop_area_u8', NULL_CALL, 'kbe_crop_area_u8: null frames_u8'),
    ('kbe_crop_area_u8', None, lambda frames: ((frames, 1.0, 4, 4, 12, 3, 3, frames, 2, 2, 6, None), (frames, 1, 4, 4, 12, 3, 3, frames, 2, 2, c_size_t(6), None),
                                               (frames, 1, 4, 4, 12, 3, 3, frames, 2, 2, 6))),
    [('kbe_crop_area_abi_version', 0, (1,)), ('kbe_crop_area_u8', 12, NULL_CALL + (0,)), ('kbe_crop_area_u8', 12, NULL_CALL[:-1])],
    ['kbe_area_reduce_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_crop_area_u8', lambda at: ((c_void_p * 2)(at, at + 1024), 2, 16, 17, 48, 15, 16, (c_void_p * 2)(at + 4096, at + 6144), 16, 4, 48, None),
     'kbe_crop_area_u8 failed (-1): kbe_crop_area_u8: w outside 1..crop_w: the entry only reduces'),
    ['kbe_crop_area_u8'], set())


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(CROP_AREA)


def test_the_library_exports_them_beside_the_others():
    thb.test_the_library_exports_them_with_the_headers_types(CROP_AREA)
    from ken_burns_effect_amd import _native, crop_area
    lib = crop_area.load()
    assert lib is _native.load() and lib.kbe_crop_area_abi_version() == 1
    for older in thb.BINDINGS:
        assert getattr(thb.module_of(older).load(), older.abi)() == 1 and thb.module_of(older).load() is lib


def test_the_older_headers_and_their_bindings_are_what_they_were():
    from ken_burns_effect_amd import _native, crop_area
    b = CROP_AREA
    crop_area.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    with open(_native.__file__) as f:
        assert b.prefix not in f.read()
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for older in thb.BINDINGS:
        other = thb.module_of(older)
        assert list(other.prototypes()) == list(older.protos) and not any(name.startswith(b.prefix) for name in other.prototypes())
        with open(other.__file__) as f:
            assert b.prefix not in f.read()
    # this is the only module of the package that names the entry
    package = os.path.dirname(crop_area.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and 'kbe_crop_area_u8' in open(os.path.join(package, name)).read()]
    assert naming == ['crop_area.py']
    name, args, text = b.null_call
    assert crop_area._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(CROP_AREA)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(CROP_AREA)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(CROP_AREA)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(CROP_AREA)


REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null out': (dict(out_u8=None), 'null out_u8'), 'n = 0': (dict(n_frames=0), 'n_frames < 1'),
           'W = 0': (dict(W=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'),
           'crop_w = 0': (dict(crop_w=0), 'crop_w outside 1..W'), 'crop_w > W': (dict(crop_w=17), 'crop_w outside 1..W'), 'crop_h > H': (dict(crop_h=18), 'crop_h outside 1..H'),
           'crop_h = -1': (dict(crop_h=-1), 'crop_h outside 1..H'), 'w > crop_w': (dict(w=15, out_stride_bytes=45), 'w outside 1..crop_w: the entry only reduces'),
           'w = 0': (dict(w=0), 'w outside 1..crop_w: the entry only reduces'), 'h > crop_h': (dict(h=14), 'h outside 1..crop_h: the entry only reduces'),
           'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'), 'out stride': (dict(out_stride_bytes=8), 'out_stride_bytes < 3 w'),
           'null frame 1': (dict(frames_u8=1), 'null element of frames_u8'), 'null output 1': (dict(out_u8=1), 'null element of out_u8')}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, crop_area
    memory = (ctypes.c_uint64 * 1024)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 2)(at, at + 1024), n_frames=2, W=16, H=17, stride_bytes=48, crop_w=14, crop_h=13, out_u8=(c_void_p * 2)(at + 4096, at + 6144), w=3, h=5,
                out_stride_bytes=9, stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key in ('frames_u8', 'out_u8') and value == 1:
            args[key][1] = None
        else:
            args[key] = value
    assert crop_area._raw('kbe_crop_area_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_crop_area_u8: ' + text
    assert not any(memory)


def test_after_a_switch_of_libraries_the_module_calls_the_new_one(monkeypatch, tmp_path):
    from ken_burns_effect_amd import _native, area, crop_area, gif
    before = _native.load()
    assert crop_area.load() is before
    variant = str(tmp_path / 'libkbe_variant.so')
    shutil.copy(_native.LIB_PATH, variant)
    for name, value in (('_lib', None), ('_kernels', None), ('LIB_PATH', variant)):
        monkeypatch.setattr(_native, name, value)
    lib = _native.load()
    assert crop_area.load() is gif.load() is area.load() is lib and lib is not before and lib._name == variant
    for module in (_native, gif, area, crop_area):
        thb.assert_typed(lib, module.prototypes())
    assert lib.kbe_crop_area_abi_version() == 1 == lib.kbe_area_abi_version() and lib.kbe_abi_version() == 13
    with pytest.raises(_native.KbeError, match='kbe_crop_area_abi_version is not an entry of include/kbe.h'):
        _native.kernels()._raw('kbe_crop_area_abi_version')
    assert crop_area._raw('kbe_crop_area_u8', *NULL_CALL) == -1 and lib.kbe_last_error().decode() == 'kbe_crop_area_u8: null frames_u8'


def test_size_for_is_area_size_for():
    from ken_burns_effect_amd import area, crop_area
    assert crop_area.size_for is area.size_for
    assert crop_area.size_for(1024, 1024, width=512) == (512, 512) and crop_area.size_for(1024, 768, width=512) == (512, 384) and crop_area.size_for(128, 96, width=50) == (50, 38)


def test_reduce_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, crop_area
    with pytest.raises(_native.KbeError):
        crop_area.reduce(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (7, 7), (3, 3))


# -- the command line and Pipeline ---------------------------------------------------------------
def test_the_command_line_takes_and_refuses_the_width():
    from ken_burns_effect_amd import kbe
    assert kbe.parse([])[0]['width'] is None
    assert kbe.parse(['--width', '512'])[0]['width'] == 512 and kbe.parse(['--width', '1'])[0]['width'] == 1
    cfg, _ = kbe.parse(['--width', '512', '--gif', '--gif-width', '512', '--write-frames'])
    assert cfg['width'] == 512 and cfg['gif-width'] == 512 and cfg['write-frames'] is True
    for argv, text in ((['--width', '0'], '--width 0: a number of pixels, 1 or more'), (['--width', '-3'], '1 or more'), (['--width', '4.5'], '--width 4.5: a number of pixels, 1 or more'),
                       (['--width', 'wide'], '1 or more'), (['--width', '480', '--gif', '--gif-width', '481'], r'--gif-width 481: the frames are 480 pixels wide \(--width\), and the GIF is only ever reduced')):
        with pytest.raises(SystemExit, match=text):
            kbe.parse(argv)


def test_out_width_and_width_size(monkeypatch):
    from ken_burns_effect_amd import pipeline, synthetic
    monkeypatch.delenv('KBE_WIDTH', raising=False)
    assert pipeline.out_width() is None and pipeline.out_width(512) == 512 and pipeline.out_width('64') == 64
    monkeypatch.setenv('KBE_WIDTH', '96')
    assert pipeline.out_width() == 96 and pipeline.out_width(32) == 32
    for bad in (0, -1, 4.5, 'wide', '4.5', '0'):
        with pytest.raises(ValueError, match=r'KBE_WIDTH, --width\): a number of pixels, 1 or more'):
            pipeline.out_width(bad)
    monkeypatch.setenv('KBE_WIDTH', 'wide')
    with pytest.raises(ValueError, match='KBE_WIDTH'):
        pipeline.out_width()
    # the default windows of a 1024 x 1024 image: the crop is 921 x 921; of 1024 x 768: 921 x 691
    ofrom, oto = synthetic.default_windows(1024, 1024)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    assert pipeline.width_size(512, 1024, 1024, zoom) == (512, 512) and pipeline.width_size(921, 1024, 1024, zoom) == (921, 921) and pipeline.width_size(1, 1024, 1024, zoom) == (1, 1)
    with pytest.raises(ValueError, match='^the crop is 921 pixels wide: outputs are only ever reduced$'):
        pipeline.width_size(922, 1024, 1024, zoom)
    # the height follows the IMAGE's aspect ratio: a crop that is flatter than the image runs out of rows first
    flat = {'objectFrom': dict(ofrom, intCropWidth=870, intCropHeight=400), 'objectTo': dict(oto, intCropWidth=800, intCropHeight=380)}
    assert pipeline.width_size(400, 1024, 1024, flat) == (400, 400)
    with pytest.raises(ValueError, match='401 pixels high and the crop is 400 pixels high: outputs are only ever reduced'):
        pipeline.width_size(401, 1024, 1024, flat)
    with pytest.raises(ValueError, match='the crop is 870 pixels wide'):
        pipeline.width_size(900, 1024, 1024, flat)


def _stub(P, width, calls, gif=None, gif_width=None):
    import torch

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = False, False, 2, {}, None, torch.device('cpu')
            self.width, self.gif, self.gif_width = width, gif, gif_width

        def estimate(self, tensorImage):
            calls.append('estimate')
            raise AssertionError('a network ran')
    return Stub()


def test_a_width_above_the_crop_is_refused_before_a_network_runs(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import kbe, pipeline
    for name in ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS'):
        monkeypatch.delenv(name, raising=False)
    calls = []
    monkeypatch.setattr(pipeline.common, 'process_kenburns', lambda *a, **k: calls.append('render'))
    image = torch.zeros(1, 3, 1024, 1024)
    zoom = kbe.windows_for(1024, 1024, dict(dict.fromkeys(('startU', 'startV', 'startH', 'endU', 'endV', 'endH')), startU=512, startV=512, endU=512, endV=512, startW=870, endW=800), False)
    assert pipeline.common.crop_size(zoom) == (870, 870)
    with pytest.raises(ValueError, match='^width 900: the crop is 870 pixels wide: outputs are only ever reduced$'):
        _stub(pipeline, 900, calls)(image, zoom, str(tmp_path / 'out'))
    with pytest.raises(ValueError, match='a number of pixels, 1 or more'):
        _stub(pipeline, 0, calls)(image, zoom, str(tmp_path / 'out'))
    with pytest.raises(ValueError, match='a GIF 481 pixels wide from frames 480 wide: the GIF is only ever reduced'):
        _stub(pipeline, 480, calls, gif=True, gif_width=481)(image, zoom, str(tmp_path / 'out'))
    monkeypatch.setenv('KBE_WIDTH', '871')
    with pytest.raises(ValueError, match='width 871: the crop is 870 pixels wide'):
        _stub(pipeline, None, calls)(image, zoom, None)
    assert calls == [] and not (tmp_path / 'out').exists()
    # the command line: the issue's message, before Pipeline is built
    monkeypatch.delenv('KBE_WIDTH')
    built = []
    monkeypatch.setattr(pipeline.Pipeline, '__init__', lambda self, *a, **k: built.append(k))
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(1024, 1024, 1)).save(path)
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        with pytest.raises(SystemExit, match='^--width 900: the crop is 870 pixels wide: outputs are only ever reduced$'):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--width', '900', '--startU', '512', '--startV', '512', '--endU', '512', '--endV', '512', '--startW', '870', '--endW', '800'])
        with pytest.raises(SystemExit, match='^--width 922: the crop is 921 pixels wide'):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--width', '922'])
    finally:
        torch.set_grad_enabled(grad)
    assert built == [] and not (tmp_path / 'out').exists()


def test_without_a_width_the_call_of_process_kenburns_is_todays(monkeypatch, tmp_path):
    """Pipeline passes out_size only when a width is set: without one process_kenburns is called with exactly the arguments it had."""
    import torch
    from ken_burns_effect_amd import pipeline, synthetic
    for name in ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_PNG', 'KBE_JPEG'):
        monkeypatch.delenv(name, raising=False)
    seen = []

    def kenburns(*args, **kw):
        seen.append(kw)
        size = kw.get('out_size', (64, 48))
        return [np.zeros((size[1], size[0], 3), np.uint8) for _ in range(2)]
    monkeypatch.setattr(pipeline.common, 'process_kenburns', kenburns)
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}

    def run(width):
        stub = _stub(pipeline, width, [])
        stub.estimate = lambda tensorImage: None
        return stub(torch.zeros(1, 3, 48, 64), zoom, None)
    assert [f.shape for f in run(None)] == [(48, 64, 3)] * 2 and seen == [{'keep_on_device': False}]
    assert [f.shape for f in run(32)] == [(24, 32, 3)] * 2 and seen[1] == {'keep_on_device': False, 'out_size': (32, 24)}


def test_process_kenburns_and_render_frames_take_out_size():
    import inspect
    from ken_burns_effect_amd import common, sharding
    assert inspect.signature(common.render_frames).parameters['out_size'].default is None
    assert inspect.signature(common.process_kenburns).parameters['out_size'].default is None
    with open(sharding.__file__) as f:
        assert 'out_size' not in f.read()                                   # (the sharded path is out of scope: it does not take the argument)
    with pytest.raises(ValueError, match='needs crop'):
        common.render_frames([], {}, None, out_size=(4, 4))


# -- what the one pass is worth ------------------------------------------------------------------
def _exact(frame, crop, size):
    """float64, nothing rounded: the bilinear half-pixel shift, then the area mean."""
    H, W, _ = frame.shape
    (cw, ch), (w, h) = crop, size
    (ipx, hx), (ipy, hy) = cc.start(W, cw), cc.start(H, ch)
    a = np.pad(frame.astype(np.float64), ((0, 1), (0, 1), (0, 0)), mode='edge')
    fx, fy = 0.5 * hx, 0.5 * hy
    tap = lambda dy, dx: a[ipy + dy:ipy + dy + ch, ipx + dx:ipx + dx + cw]                                                  # noqa: E731
    patch = (1 - fy) * ((1 - fx) * tap(0, 0) + fx * tap(0, 1)) + fy * ((1 - fx) * tap(1, 0) + fx * tap(1, 1))
    return np.einsum('oy,yxc,px->opc', ac.weights(h, ch).astype(np.float64), patch, ac.weights(w, cw).astype(np.float64), optimize=True) / (cw * ch)


def _psnr(got, want):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((got.astype(np.float64) - want) ** 2))


def test_one_pass_beside_reducing_the_enlarged_frames(oracle):
    """Quality, recorded and not a bar.  Two routes to a narrower frame, both against the float64 restatement of "bilinear half-pixel shift,
    then area mean" with nothing rounded: this one (patch, then area mean: two roundings), and the composition a user of the frames written
    today would get (crop + resize back to W x H -- the oracle's twin of kbe_crop_resize_u8 --, then the area twin: three resamplings).

    Measured, PSNR in dB, two photo_like 160 x 128 frames each (one pass / enlarge then reduce):
        crop            -> 80x64            -> 75x60            -> 40x32
        ee 156x122      57.5-57.6 / 56.6-56.7   57.6-57.7 / 52.0-52.1   58.0 / 58.2-58.3
        oe 155x124      56.2 / 55.6             56.1 / 51.8-51.9        56.4-56.5 / 57.4
        eo 156x125      56.1-56.2 / 55.7        56.2 / 51.7-51.9        56.4 / 57.4
        oo 155x125      58.9 / 58.0-58.1        58.9 / 51.6-51.7        58.9-59.0 / 58.1-58.3
        full 160x128    the same bytes: the enlargement of a full-size crop is the patch itself
    The one pass is the closer by 0.5-0.9 dB at a factor of 2 and by 4-7 dB at a ratio that is no integer, where the composition's second
    resampling does not fall on whole pixels of its first.  At a factor of 4 from a crop that starts on a half pixel the composition is the
    closer by 0.2-1.1 dB: both are then within a third of a count of the exact value on average, and the one pass pays the rounding of its
    patch to bytes.  So the first figure is not the larger on every frame tried, and nothing is asserted about the figures."""
    W, H = cc.FRAMES[2]
    for name in ('ee', 'oe', 'eo', 'oo', 'full'):
        crop = cc.crop_of((W, H), name)
        for frame in cc.frames(W, H):
            enlarged = oracle.crop_resize_u8(np.ascontiguousarray(frame), *crop)
            for size in ((W // 2, H // 2), (75, 60), (W // 4, H // 4)):
                want = _exact(frame, crop, size)
                one, two = _psnr(cc.twin_reduce(frame, crop, size), want), _psnr(ac.twin_reduce(enlarged, *size), want)
                print('%s crop %dx%d -> %dx%d: one pass %.2f dB, enlarge then reduce %.2f dB' % (name, crop[0], crop[1], size[0], size[1], one, two))
                assert np.isfinite(one) and np.isfinite(two)
