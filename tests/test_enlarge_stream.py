"""The crop + exact bicubic enlargement (include/kbe_enlarge.h) without a GPU: csrc/kbe_enlarge_block.h executed serially under its sanitizers
(tests/enlarge_check.cpp) against coefficients as exact rationals and against the NumPy twin (tests/enlarge_cases.py); the twin's properties
and its distance to Pillow's bicubic; the binding (enlarge.py) held to what tests/test_header_bindings.py holds the older headers to; and the
command line's --enlarge and Pipeline(enlarge=)."""
import ctypes
import importlib
import os
import re
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest
from PIL import Image

import crop_area_cases as cc
import enlarge_cases as ec
import gif_cases as gc
import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY = r': axes (\d+), indices (\d+), bad positions (\d+), bad floors (\d+), bad sums (\d+), bad taps (\d+), bad identities (\d+), negative (\d+), lowest (-?\d+), highest (-?\d+)'
ids = lambda v: v if isinstance(v, str) else '%dx%d' % v                     # noqa: E731


# -- the definition ---------------------------------------------------------------------------
def test_the_header_against_exact_rationals():
    """enlarge_check.cpp builds under -fsanitize=signed-integer-overflow,address, and taps() of csrc/kbe_enlarge_block.h equals the weights as
    __int128 rationals at every n_in <= n_out <= 12: 78 axes, 650 indices; the sums are 16384, a floor is a floor of a negative numerator too
    (some are negative), and n_out == n_in gives (0, 16384, 0, 0)."""
    axes, indices, *bad, negative, lowest, highest = (int(v) for v in re.search('brute' + TALLY, ec.ask('brute', 12)).groups())
    assert (axes, indices) == (78, 650) and bad == [0] * 5 and negative > 0 and -ec.ONE // 8 < lowest < 0 and highest == ec.ONE


def test_the_int64_bounds_worst_cases_end_clean_under_the_sanitizer():
    """Every x of 16383 -> 16384, 1 -> 16384 and 16384 -> 16384: no signed overflow (the program would have aborted), and the exact rationals."""
    axes, indices, *bad, negative, lowest, highest = (int(v) for v in re.search('limits' + TALLY, ec.ask('limits')).groups())
    assert (axes, indices) == (3, 3 * 16384) and bad == [0] * 5 and negative > 0 and highest == ec.ONE
    c, t = ec.axis(16383, 16384)
    assert (c.sum(axis=1) == ec.ONE).all() and (int(c.min()), int(c.max())) == (lowest, highest)


def test_the_coefficients_of_the_twin():
    for n_in, n_out in ((870, 16384), (115, 256), (1, 5), (2, 9), (33, 700), (50, 50)):
        c, t = ec.axis(n_in, n_out)
        assert (c.sum(axis=1) == ec.ONE).all() and t.min() == 0 and t.max() == n_in - 1 and (np.diff(t, axis=0) >= 0).all()
    c, t = ec.axis(870, 16384)
    assert (int(c.min()), int(c.max())) == (-1214, 16384)
    c, t = ec.axis(50, 50)
    assert (c == (0, ec.ONE, 0, 0)).all() and (t[:, 1] == np.arange(50)).all()


@pytest.mark.parametrize('frame, name', ec.EVERY_CROP, ids=ids)
def test_the_header_is_the_twin(frame, name):
    """enlarge_pixel of csrc/kbe_enlarge_block.h on the GPU suite's frames, rows padded: the NumPy twin byte for byte, at every target."""
    crop = ec.crop_of(frame, name)
    for size in ec.targets(crop).values():
        assert np.array_equal(ec.header_enlarge(ec.frames(*frame), crop, size, pad=5), ec.twin_of(frame[0], frame[1], crop, size)), (crop, size)


@pytest.mark.parametrize('frame, crop', ec.SMALL, ids=ids)
def test_the_header_is_the_twin_sevenfold(frame, crop):
    size = (7 * crop[0], 7 * crop[1])
    assert np.array_equal(ec.header_enlarge(ec.frames(*frame), crop, size), ec.twin_of(frame[0], frame[1], crop, size))


def test_the_header_is_the_twin_on_degenerate_crops_and_many_tiles():
    frame = ec.frames(37, 50)
    for crop, size in (((1, 1), (5, 3)), ((2, 2), (9, 9)), ((33, 5), (700, 11)), ((5, 33), (11, 700))):
        assert np.array_equal(ec.header_enlarge(frame, crop, size), ec.twin_enlarge(frame, crop, size)), (crop, size)


# -- properties of the twin --------------------------------------------------------------------
@pytest.mark.parametrize('frame, name', ec.EVERY_CROP, ids=ids)
def test_the_crops_own_size_gives_the_patch_itself(frame, name):
    crop = ec.crop_of(frame, name)
    patch = cc.twin_patch(ec.frames(*frame), *crop)
    assert np.array_equal(ec.twin_enlarge(ec.frames(*frame), crop, crop), patch)
    assert np.array_equal(ec.header_enlarge(ec.frames(*frame), crop, crop), patch)


def test_a_constant_frame_stays_constant():
    for value in (0, 1, 137, 254, 255):
        for (W, H), name in ((ec.FRAMES[0], 'ee'), (ec.FRAMES[1], 'oe'), (ec.FRAMES[1], 'full'), (ec.FRAMES[2], 'eo')):
            crop = ec.crop_of((W, H), name)
            for size in ec.targets(crop).values():
                assert (ec.twin_enlarge(np.full((H, W, 3), value, np.uint8), crop, size) == value).all()
    assert (ec.twin_enlarge(ec.frames(37, 50), (1, 1), (5, 3)) == cc.twin_patch(ec.frames(37, 50), 1, 1)).all()


def test_both_clamps_of_both_passes_are_exercised():
    """A 0 / 255 checkerboard, a crop on whole pixels (the patch is the board): the twin counts unclamped sums below 0 and above 255 in the
    pass along the rows and in the pass down the columns, and the header clamps them to the same bytes."""
    board = ec.checkerboard(37, 50)
    counts = []
    want = ec.twin_enlarge(board, (32, 47), (61, 90), counts)
    assert len(counts) == 2 and all(below > 0 and above > 0 for below, above in counts), counts
    assert np.array_equal(ec.header_enlarge(board[None], (32, 47), (61, 90))[0], want) and want.min() == 0 and want.max() == 255


def test_a_frames_bytes_do_not_depend_on_its_neighbours():
    W, H = ec.FRAMES[2]
    five = ec.frames(W, H, 5)
    crop = ec.crop_of((W, H), 'ee')
    size = ec.targets(crop)['under_2']
    together = ec.twin_enlarge(five, crop, size)
    for i in (0, 2, 4):
        assert np.array_equal(ec.twin_enlarge(five[i], crop, size), together[i])
        assert np.array_equal(ec.twin_enlarge(five[[4 - i, i, 2]], crop, size)[1], together[i])
    assert np.array_equal(ec.header_enlarge(five[[3, 1]], crop, size)[1], together[1])


PILLOW_CASES = [((115, 86), (256, 192)), ((37, 50), (38, 51)), ((64, 48), (64, 48)), ((33, 44), (200, 267)), ((870, 580), (1920, 1280))]


def test_the_distance_to_pillows_bicubic():
    """A condition on the twin, not on the device.  Pillow's Image.BICUBIC is the same kernel with 22-bit coefficients, both passes in one
    rounding chain of its own and borders renormalised instead of clamped: on uniform noise the interior -- without 2 ceil(n_out / n_in) + 1
    pixels at each edge -- differs by at most 2 counts and on fewer than 2 % of the values.  Measured with Pillow 12.2.0: 2, 1, 0, 1, 1 counts
    and 0.52, 0.23, 0, 0.46, 0.59 %."""
    rng = np.random.default_rng(0)
    for (cw, ch), (w, h) in PILLOW_CASES:
        noise = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
        mine = ec.twin_resample(noise, (w, h)).astype(np.int64)
        theirs = np.asarray(Image.fromarray(noise).resize((w, h), Image.BICUBIC)).astype(np.int64)
        mx, my = 2 * -(-w // cw) + 1, 2 * -(-h // ch) + 1
        apart = np.abs(mine - theirs)[my:h - my, mx:w - mx]
        print('%dx%d -> %dx%d: at most %d counts, %.2f %% of the interior, %d at the borders' % (cw, ch, w, h, apart.max(), 100.0 * (apart != 0).mean(), np.abs(mine - theirs).max()))
        assert apart.size and apart.max() <= 2 and (apart != 0).mean() < 0.02


# -- the binding -------------------------------------------------------------------------------
p, i = c_void_p, c_int
NULL_CALL = (None, 1, 4, 4, 12, 3, 3, None, 5, 5, 15, None)
OLDER = [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
         ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n'), ('kbe_dof.h', '#define KBE_DOF_ABI_VERSION 1\n'), ('kbe_shutter.h', '#define KBE_SHUTTER_ABI_VERSION 1\n'),
         ('kbe_yuv.h', '#define KBE_YUV_ABI_VERSION 1\n'), ('kbe_transition.h', '#define KBE_TRANSITION_ABI_VERSION 1\n'), ('kbe_overlay.h', '#define KBE_OVERLAY_ABI_VERSION 1\n'),
         ('kbe_grade.h', '#define KBE_GRADE_ABI_VERSION 1\n')]
ENLARGE = thb.Binding(
    'enlarge', 'kbe_enlarge',
    # frames, n, W, H, stride; crop w, crop h; out, w, h, out stride; stream
    {'kbe_enlarge_abi_version': (c_int, []), 'kbe_enlarge_u8': (c_int, [p, i, i, i, i, i, i, p, i, i, i, p])},
    'kbe_enlarge_abi_version', ['#define KBE_ENLARGE_ABI_VERSION 1\n'], ['KBE_ENLARGE_BGR'], {'ABI_VERSION': 1, 'MAX_SIDE': 16384},
    OLDER,
    ('kbe_enlarge_u8', NULL_CALL, 'kbe_enlarge_u8: null frames_u8'),
    ('kbe_enlarge_u8', None, lambda frames: ((frames, 1.0, 4, 4, 12, 3, 3, frames, 5, 5, 15, None), (frames, 1, 4, 4, 12, 3, 3, frames, 5, 5, c_size_t(15), None),
                                             (frames, 1, 4, 4, 12, 3, 3, frames, 5, 5, 15))),
    [('kbe_enlarge_abi_version', 0, (1,)), ('kbe_enlarge_u8', 12, NULL_CALL + (0,)), ('kbe_enlarge_u8', 12, NULL_CALL[:-1])],
    ['kbe_crop_area_u8', 'kbe_area_reduce_u8', 'kbe_grade_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_enlarge_u8', lambda at: ((c_void_p * 2)(at, at + 1024), 2, 16, 17, 48, 15, 16, (c_void_p * 2)(at + 4096, at + 6144), 14, 20, 42, None),
     'kbe_enlarge_u8 failed (-1): kbe_enlarge_u8: w outside crop_w..16384: the entry only enlarges'),
    ['kbe_enlarge_u8'], set())
# what the other headers' modules declare: the lists this header must leave as they are
OTHERS = {'gif': list(thb.GIF.protos), 'area': list(thb.AREA.protos), 'crop_area': ['kbe_crop_area_abi_version', 'kbe_crop_area_u8'], 'dof': ['kbe_dof_abi_version', 'kbe_dof_u8'],
          'shutter': ['kbe_shutter_abi_version', 'kbe_shutter_mean_u8'], 'yuv': ['kbe_yuv_abi_version', 'kbe_yuv420_bytes', 'kbe_yuv420_u8'],
          'transition': ['kbe_transition_abi_version', 'kbe_transition_u8'], 'overlay': ['kbe_overlay_abi_version', 'kbe_overlay_u8'], 'grade': ['kbe_grade_abi_version', 'kbe_grade_u8']}


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(ENLARGE)
    from ken_burns_effect_amd import enlarge
    assert list(enlarge.prototypes()) == ['kbe_enlarge_abi_version', 'kbe_enlarge_u8']


def test_the_library_exports_them_beside_the_others():
    thb.test_the_library_exports_them_with_the_headers_types(ENLARGE)
    from ken_burns_effect_amd import _native, enlarge
    lib = enlarge.load()
    assert lib is _native.load() and lib.kbe_enlarge_abi_version() == 1 == enlarge.ABI_VERSION
    for name, entries in OTHERS.items():
        module = importlib.import_module('ken_burns_effect_amd.' + name)
        assert module.load() is lib and getattr(lib, entries[0])() == 1


def test_the_older_headers_and_their_bindings_are_what_they_were():
    from ken_burns_effect_amd import _native, enlarge
    b = ENLARGE
    enlarge.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for name, entries in OTHERS.items():
        other = importlib.import_module('ken_burns_effect_amd.' + name)
        assert list(other.prototypes()) == entries and other.ABI_VERSION == 1
    # enlarge.py is the only module of the package whose text names the header's prefix, and it names no entry of another header
    package = os.path.dirname(enlarge.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and b.prefix in open(os.path.join(package, name)).read()]
    assert naming == ['enlarge.py']
    with open(enlarge.__file__) as f:
        text = f.read()
    foreign = set(_native.SYMBOLS) | {entry for entries in OTHERS.values() for entry in entries}
    assert not [entry for entry in sorted(foreign) if entry in text]
    name, args, text = b.null_call
    assert enlarge._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(ENLARGE)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(ENLARGE)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(ENLARGE)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(ENLARGE)


def test_the_makefile_builds_the_source():
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'Makefile')) as f:
        text = f.read()
    assert ' kbe_enlarge.hip' in text and ' kbe_enlarge_block.h' in text and '../../include/kbe_enlarge.h' in text


REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null out': (dict(out_u8=None), 'null out_u8'), 'n = 0': (dict(n_frames=0), 'n_frames < 1'),
           'W = 0': (dict(W=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'),
           'crop_w = 0': (dict(crop_w=0), 'crop_w outside 1..W'), 'crop_w > W': (dict(crop_w=17), 'crop_w outside 1..W'), 'crop_h > H': (dict(crop_h=18), 'crop_h outside 1..H'),
           'crop_h = -1': (dict(crop_h=-1), 'crop_h outside 1..H'), 'w < crop_w': (dict(w=13), 'w outside crop_w..16384: the entry only enlarges'),
           'w = 16385': (dict(w=16385, out_stride_bytes=3 * 16385), 'w outside crop_w..16384: the entry only enlarges'),
           'h < crop_h': (dict(h=12), 'h outside crop_h..16384: the entry only enlarges'), 'h = 16385': (dict(h=16385), 'h outside crop_h..16384: the entry only enlarges'),
           'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'), 'out stride': (dict(out_stride_bytes=89), 'out_stride_bytes < 3 w'),
           'null frame 1': (dict(frames_u8=1), 'null element of frames_u8'), 'null output 1': (dict(out_u8=1), 'null element of out_u8')}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, enlarge
    memory = (ctypes.c_uint64 * 1024)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 2)(at, at + 1024), n_frames=2, W=16, H=17, stride_bytes=48, crop_w=14, crop_h=13, out_u8=(c_void_p * 2)(at + 4096, at + 6144), w=30, h=20,
                out_stride_bytes=90, stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key in ('frames_u8', 'out_u8') and value == 1:
            args[key][1] = None
        else:
            args[key] = value
    assert enlarge._raw('kbe_enlarge_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_enlarge_u8: ' + text
    assert not any(memory)


def test_enlarge_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, enlarge
    with pytest.raises(_native.KbeError):
        enlarge.enlarge(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (7, 7), (9, 9))
    assert enlarge.size_for(1024, 768, width=1920) == (1920, 1440)


# -- the command line and Pipeline ---------------------------------------------------------------
def test_the_command_line_takes_the_switch():
    from ken_burns_effect_amd import kbe, slideshow
    assert kbe.parse([])[0]['enlarge'] is False and kbe.parse(['--width', '512'])[0]['enlarge'] is False
    cfg, _ = kbe.parse(['--width', '1920', '--enlarge', '--gif', '--gif-width', '1920'])
    assert cfg['enlarge'] is True and cfg['width'] == 1920 and cfg['gif-width'] == 1920
    with pytest.raises(SystemExit, match='^--enlarge: only with --width$'):
        kbe.parse(['--enlarge'])
    with pytest.raises(SystemExit, match=r'--gif-width 1921: the frames are 1920 pixels wide \(--width\), and the GIF is only ever reduced'):
        kbe.parse(['--width', '1920', '--enlarge', '--gif', '--gif-width', '1921'])
    assert 'enlarge' in kbe.LONG_OPTIONS and 'enlarge=' not in kbe.LONG_OPTIONS and '[--enlarge]' in kbe.__doc__ and 'KBE_ENLARGE=1' in kbe.__doc__
    assert 'enlarge' in slideshow.LONG_OPTIONS and '[--enlarge]' in slideshow.__doc__
    assert slideshow.parse(['--in', 'a.png', '--width', '1920', '--enlarge'])['enlarge'] is True
    with pytest.raises(SystemExit, match='--enlarge: only with --width'):
        slideshow.parse(['--in', 'a.png', '--enlarge'])


def test_enlarge_switch_and_width_size(monkeypatch):
    from ken_burns_effect_amd import pipeline, synthetic
    monkeypatch.delenv('KBE_ENLARGE', raising=False)
    assert pipeline.enlarge_switch() is False and pipeline.enlarge_switch(True) is True and pipeline.enlarge_switch(0) is False
    monkeypatch.setenv('KBE_ENLARGE', '1')
    assert pipeline.enlarge_switch() is True and pipeline.enlarge_switch(False) is False
    # the default windows of a 1024 x 1024 image: the crop is 921 x 921
    ofrom, oto = synthetic.default_windows(1024, 1024)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    assert pipeline.width_size(1920, 1024, 1024, zoom, enlarge=True) == (1920, 1920) and pipeline.grows((1920, 1920), zoom)
    assert pipeline.width_size(3684, 1024, 1024, zoom, enlarge=True) == (3684, 3684)
    assert pipeline.width_size(512, 1024, 1024, zoom, enlarge=True) == (512, 512) == pipeline.width_size(512, 1024, 1024, zoom) and not pipeline.grows((512, 512), zoom)
    assert pipeline.width_size(921, 1024, 1024, zoom, enlarge=True) == (921, 921) and not pipeline.grows((921, 921), zoom)
    with pytest.raises(ValueError, match='^the crop is 921 pixels wide: outputs are enlarged at most 4-fold, to 3684$'):
        pipeline.width_size(3685, 1024, 1024, zoom, enlarge=True)
    with pytest.raises(ValueError, match='^the crop is 921 pixels wide: outputs are only ever reduced$'):
        pipeline.width_size(922, 1024, 1024, zoom)
    # a crop flatter than the image: 870 x 400 of 1024 x 1024.  --width 500 gives 500 x 500: the width shrinks and the height grows
    flat = {'objectFrom': dict(ofrom, intCropWidth=870, intCropHeight=400), 'objectTo': dict(oto, intCropWidth=800, intCropHeight=380)}
    with pytest.raises(ValueError, match='^the outputs are then 500x500 and the crop is 870x400: one side would grow and the other shrink$'):
        pipeline.width_size(500, 1024, 1024, flat, enlarge=True)
    assert pipeline.width_size(400, 1024, 1024, flat, enlarge=True) == (400, 400) and pipeline.width_size(870, 1024, 1024, flat, enlarge=True) == (870, 870)
    # a tall crop of a huge image: four times its width is allowed, 16384 pixels a side are not exceeded
    tall = {'objectFrom': dict(ofrom, intCropWidth=5000, intCropHeight=5000), 'objectTo': dict(oto, intCropWidth=5000, intCropHeight=5000)}
    with pytest.raises(ValueError, match='the outputs are then 16385x16385: an enlarged side is at most 16384 pixels'):
        pipeline.width_size(16385, 8192, 8192, tall, enlarge=True)


def _stub(P, width, calls, enlarge=None):
    import torch

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = False, False, 2, {}, None, torch.device('cpu')
            self.width, self.enlarge = width, enlarge

        def estimate(self, tensorImage):
            calls.append('estimate')
            raise AssertionError('a network ran')
    return Stub()


ZOOM_870 = dict(dict.fromkeys(('startU', 'startV', 'startH', 'endU', 'endV', 'endH')), startU=512, startV=512, endU=512, endV=512, startW=870, endW=800)
CLI_870 = ['--startU', '512', '--startV', '512', '--endU', '512', '--endV', '512', '--startW', '870', '--endW', '800']


def test_the_refusals_come_before_a_network_runs(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import kbe, pipeline
    for name in ('KBE_WIDTH', 'KBE_ENLARGE', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS'):
        monkeypatch.delenv(name, raising=False)
    calls = []
    monkeypatch.setattr(pipeline.common, 'process_kenburns', lambda *a, **k: calls.append('render'))
    image = torch.zeros(1, 3, 1024, 1024)
    zoom = kbe.windows_for(1024, 1024, ZOOM_870, False)
    assert pipeline.common.crop_size(zoom) == (870, 870)
    out = str(tmp_path / 'out')
    with pytest.raises(ValueError, match='^width 3481: the crop is 870 pixels wide: outputs are enlarged at most 4-fold, to 3480$'):
        _stub(pipeline, 3481, calls, enlarge=True)(image, zoom, out)
    with pytest.raises(ValueError, match=r'^enlarge \(KBE_ENLARGE, --enlarge\): only with a width$'):
        _stub(pipeline, None, calls, enlarge=True)(image, zoom, out)
    # without the switch: today's text, from the instance and from the environment
    with pytest.raises(ValueError, match='^width 900: the crop is 870 pixels wide: outputs are only ever reduced$'):
        _stub(pipeline, 900, calls)(image, zoom, out)
    with pytest.raises(ValueError, match='^width 900: the crop is 870 pixels wide: outputs are only ever reduced$'):
        _stub(pipeline, 900, calls, enlarge=False)(image, zoom, out)
    monkeypatch.setenv('KBE_ENLARGE', '1')
    monkeypatch.setenv('KBE_WIDTH', '3481')
    with pytest.raises(ValueError, match='width 3481: the crop is 870 pixels wide: outputs are enlarged at most 4-fold'):
        _stub(pipeline, None, calls)(image, zoom, None)
    with pytest.raises(ValueError, match='at most 4-fold'):
        _stub(pipeline, None, calls).render(image, zoom)
    monkeypatch.delenv('KBE_ENLARGE')
    monkeypatch.delenv('KBE_WIDTH')
    assert calls == [] and not (tmp_path / 'out').exists()
    # the command line: before Pipeline is built
    built = []
    monkeypatch.setattr(pipeline.Pipeline, '__init__', lambda self, *a, **k: built.append(k))
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(1024, 1024, 1)).save(path)
    flat = ['--startU', '512', '--startV', '512', '--endU', '512', '--endV', '512', '--startW', '870', '--startH', '400', '--endW', '800', '--endH', '380']
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        with pytest.raises(SystemExit, match='^--width 9000: the crop is 870 pixels wide: outputs are enlarged at most 4-fold, to 3480$'):
            kbe.main(['--in', path, '--out', out, '--width', '9000', '--enlarge'] + CLI_870)
        with pytest.raises(SystemExit, match='^--width 500: the outputs are then 500x500 and the crop is 870x400: one side would grow and the other shrink$'):
            kbe.main(['--in', path, '--out', out, '--width', '500', '--enlarge'] + flat)
        with pytest.raises(SystemExit, match='^--width 900: the crop is 870 pixels wide: outputs are only ever reduced$'):
            kbe.main(['--in', path, '--out', out, '--width', '900'] + CLI_870)
        with pytest.raises(SystemExit, match='^--enlarge: only with --width$'):
            kbe.main(['--in', path, '--out', out, '--enlarge'] + CLI_870)
    finally:
        torch.set_grad_enabled(grad)
    assert built == [] and not (tmp_path / 'out').exists()


def test_the_keyword_is_absent_from_a_call_that_did_not_ask_for_it(monkeypatch):
    """Pipeline passes enlarge=True only where the frames grow: without the switch, and with it at a width within the crop, process_kenburns
    is called with exactly the arguments it had."""
    import torch
    from ken_burns_effect_amd import pipeline, synthetic
    for name in ('KBE_WIDTH', 'KBE_ENLARGE', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_PNG', 'KBE_JPEG'):
        monkeypatch.delenv(name, raising=False)
    seen = []

    def kenburns(*args, **kw):
        seen.append(kw)
        size = kw.get('out_size', (64, 48))
        frames = np.zeros((2, size[1], size[0], 3), np.uint8)
        return torch.from_numpy(frames) if kw['keep_on_device'] else list(frames)
    monkeypatch.setattr(pipeline.common, 'process_kenburns', kenburns)
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    assert pipeline.common.crop_size(zoom) == (57, 43)

    def run(width, enlarge, render=False):
        stub = _stub(pipeline, width, [], enlarge)
        stub.estimate = lambda tensorImage: None
        return stub.render(torch.zeros(1, 3, 48, 64), zoom) if render else stub(torch.zeros(1, 3, 48, 64), zoom, None)
    assert [f.shape for f in run(None, None)] == [(48, 64, 3)] * 2 and seen == [{'keep_on_device': False}]
    assert [f.shape for f in run(32, None)] == [(24, 32, 3)] * 2 and seen[1] == {'keep_on_device': False, 'out_size': (32, 24)}
    assert [f.shape for f in run(32, True)] == [(24, 32, 3)] * 2 and seen[2] == {'keep_on_device': False, 'out_size': (32, 24)}
    assert [f.shape for f in run(128, True)] == [(96, 128, 3)] * 2 and seen[3] == {'keep_on_device': False, 'out_size': (128, 96), 'enlarge': True}
    monkeypatch.setenv('KBE_ENLARGE', '1')
    monkeypatch.setenv('KBE_WIDTH', '200')
    assert [f.shape for f in run(None, None)] == [(150, 200, 3)] * 2 and seen[4] == {'keep_on_device': False, 'out_size': (200, 150), 'enlarge': True}
    assert tuple(run(None, None, render=True).shape) == (2, 150, 200, 3) and seen[5] == {'keep_on_device': True, 'out_size': (200, 150), 'enlarge': True}


def test_process_kenburns_and_render_frames_take_the_keyword():
    import inspect
    from ken_burns_effect_amd import common, sharding
    for fn in (common.render_frames, common.process_kenburns, common._render_reduced, common._render_lens, common._render_shutter):
        assert inspect.signature(fn).parameters['enlarge'].default is False
    with open(sharding.__file__) as f:
        assert 'enlarge' not in f.read()                                    # (the sharded path is out of scope: it does not learn the option)
    with pytest.raises(ValueError, match='needs crop'):
        common.render_frames([], {}, None, out_size=(4, 4), enlarge=True)
    with pytest.raises(ValueError, match='needs out_size'):
        common.render_frames([], {}, (3, 3), enlarge=True)


def test_a_slideshow_takes_the_switch():
    from ken_burns_effect_amd import slideshow
    show = slideshow.checked([(1024, 1024), (1024, 1024)], 75, width=1920, enlarge=True)
    assert show['size'] == (1920, 1920)
    assert slideshow.checked([(1024, 1024)], 75, width=512, enlarge=True)['size'] == (512, 512) == slideshow.checked([(1024, 1024)], 75, width=512)['size']
    with pytest.raises(ValueError, match='^--width 1920: photo 0: the crop is 921 pixels wide: outputs are only ever reduced$'):
        slideshow.checked([(1024, 1024)], 75, width=1920)
    with pytest.raises(ValueError, match='^--width 3685: photo 0: the crop is 921 pixels wide: outputs are enlarged at most 4-fold, to 3684$'):
        slideshow.checked([(1024, 1024)], 75, width=3685, enlarge=True)
    with pytest.raises(ValueError, match='^--enlarge: only with --width$'):
        slideshow.checked([(1024, 1024)], 75, enlarge=True)
