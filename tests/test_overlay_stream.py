"""The overlay (include/kbe_overlay.h) without a GPU: csrc/kbe_overlay_block.h executed serially (tests/overlay_check.cpp) against the plain
definition and against the NumPy twin (tests/overlay_cases.py) on the GPU suite's cases; the pinned values; the binding (overlay.py) held to
what tests/test_header_bindings.py holds the older headers to; every refusal of the entry on host memory; place, opacity_table and the
slideshow's caption windows against hand-written values; caption_image against its `over` formula on Pillow's own mask; and every refusal
of the two command lines, raised before a network is built."""
import ctypes
import os
import re
from ctypes import c_int, c_int32, c_size_t, c_void_p

import numpy as np
import pytest
from PIL import Image

import gif_cases as gc
import overlay_cases as oc
import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition ---------------------------------------------------------------------------
def test_the_packed_forms_are_the_plain_one():
    """overlay_check.cpp builds; all 256^3 (c, o, e), packed against plain, the division without a divide; all 256 x 257 (a, opacity), through
    a whole piece at every channel phase; x = j / 3 for every first byte; the colour stream; rows lane by lane at all 64 pairs of
    alignment classes and ten widths.  All mismatch counts are zero."""
    m = re.search(r'brute: overs (\d+), plain mismatches (\d+), packed mismatches (\d+), alphas (\d+), alpha mismatches (\d+), thirds (\d+), third mismatches (\d+), '
                  r'stream mismatches (\d+), rows (\d+), row mismatches (\d+)', oc.ask('brute'))
    overs, plain, packed, alphas, alpha_bad, thirds, third_bad, stream_bad, rows, row_bad = (int(v) for v in m.groups())
    assert overs == 256 ** 3 and alphas == 256 * 257 and thirds == 3 * 65535 + 15 and rows == 10 * 16 * 4
    assert (plain, packed, alpha_bad, third_bad, stream_bad, row_bad) == (0,) * 6


def _flat(v, shape=(1, 3, 5, 3)):
    return np.full(shape, v, np.uint8)


def test_the_pinned_values():
    """The pinned values of e and of out, for the twin, and for the header through flat frames under a flat overlay."""
    assert [int(oc.effective(a, p)) for a, p in ((255, 256), (255, 128), (255, 1), (128, 128), (1, 127), (1, 128), (0, 256), (200, 0))] == [255, 128, 1, 64, 0, 1, 0, 0]
    pinned = (((0, 255, 255, 128), 128), ((255, 0, 255, 1), 254), ((0, 255, 255, 255), 254), ((10, 20, 64, 256), 13), ((200, 100, 128, 256), 150), ((7, 250, 255, 256), 250),
              ((7, 250, 0, 256), 7), ((7, 250, 255, 0), 7), ((0, 255, 1, 256), 1), ((255, 0, 1, 256), 254))
    for (c, o, a, opacity), want in pinned:
        assert oc.over(c, o, oc.effective(a, opacity)) == want
        picture = np.concatenate([_flat(o, (2, 4, 3)), _flat(a, (2, 4, 1))], axis=2)
        for over in (oc.twin_over, oc.header_over):
            got = over(_flat(c), picture, 1, 1, opacity)
            assert (got[0, 1:, 1:] == want).all() and (got[0, 0] == c).all() and (got[0, :, 0] == c).all(), (c, o, a, opacity, over.__name__)
    c, o, e = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing='ij')
    out = oc.over(c, o, e)
    assert np.array_equal(out[:, :, 0], c[:, :, 0]) and np.array_equal(out[:, :, 255], o[:, :, 255]) and np.array_equal(out[c == o], c[c == o])
    assert (np.abs(255 * out - (c * (255 - e) + o * e)) <= 127).all() and 255 * 255 + 127 == 65152 < 1 << 16


@pytest.mark.parametrize('frame', oc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_header_is_the_twin(frame):
    """over_row of csrc/kbe_overlay_block.h on the GPU suite's frames, the frames' rows padded by 5 and the overlay's by 1 (every row at another
    alignment): the NumPy twin byte for byte, on inputs that tell."""
    W, H = frame
    frames, picture = oc.frames_of(W, H), oc.overlay_of(*oc.OVERLAY)
    want = oc.twin_of(W, H)
    assert np.array_equal(oc.header_over(frames, picture, oc.X, oc.Y, oc.OPACITY, pad=5, overlay_pad=1), want)
    assert all((want[i] != frames[i]).any(axis=2).sum() > 21 * 9 // 2 for i in (0, 1)) and {0, 255} <= set(np.unique(picture[:, :, 3]).tolist())
    inside = np.zeros((2, H, W), bool)
    for i in (0, 1):
        inside[i, oc.Y[i]:oc.Y[i] + 9, oc.X[i]:oc.X[i] + 21] = True
    assert np.array_equal(want[~inside], frames[~inside])


CLIPPED = [(-5, 3), (30, 3), (3, -4), (3, 45), (-5, -4), (30, -4), (-5, 45), (30, 45), (36, 49), (-20, -8), (37, 3), (-21, 3), (3, 50), (3, -9), (65535, -65535)]


def test_the_header_clips_as_the_twin_does():
    """Off each edge and corner of a 37x50 frame, wholly outside and exactly touching; an overlay larger than the frame; overlays of 1, 2 and 5
    pixels and one row; a frame one pixel wide; rows of 4098 bytes."""
    frames, picture = oc.frames_of(37, 50, len(CLIPPED)), oc.overlay_of(*oc.OVERLAY)
    xs, ys = zip(*CLIPPED)
    want = oc.twin_over(frames, picture, xs, ys, 200)
    assert np.array_equal(oc.header_over(frames, picture, xs, ys, 200, pad=3, overlay_pad=3), want)
    assert all(np.array_equal(want[i], frames[i]) for i in range(10, 15)) and all((want[i] != frames[i]).any() for i in range(8))
    big = oc.overlay_of(80, 70)
    assert np.array_equal(oc.header_over(frames[:2], big, (-13, -43), (-7, -20), 256, pad=1), oc.twin_over(frames[:2], big, (-13, -43), (-7, -20), 256))
    for w, h in ((1, 9), (2, 9), (5, 9), (21, 1)):
        small = oc.overlay_of(w, h)
        xs, ys = list(range(3, 18)), [(5 * i) % 11 for i in range(15)]
        assert np.array_equal(oc.header_over(frames, small, xs, ys, 230, pad=2, overlay_pad=1), oc.twin_over(frames, small, xs, ys, 230))
    thin = oc.frames_of(1, 7)
    assert np.array_equal(oc.header_over(thin, oc.overlay_of(5, 2), (0, -3), (0, 1), 256, pad=3), oc.twin_over(thin, oc.overlay_of(5, 2), (0, -3), (0, 1), 256))
    wide = oc.frames_of(1366, 3)
    assert np.array_equal(oc.header_over(wide, oc.overlay_of(1366, 2), 0, (0, 1), (256, 77), pad=1), oc.twin_over(wide, oc.overlay_of(1366, 2), 0, (0, 1), (256, 77)))


def test_the_extremes_of_the_header():
    frames = oc.frames_of(37, 12, 3)
    clear, solid = oc.overlay_of(21, 9, alpha=0), oc.overlay_of(21, 9, alpha=255)
    assert np.array_equal(oc.header_over(frames, clear, 4, 2, (256, 255, 1)), frames) and np.array_equal(oc.header_over(frames, solid, 4, 2, 0), frames)
    got = oc.header_over(frames, solid, 4, 2, 256)
    assert all(np.array_equal(got[i, 2:11, 4:25], solid[:, :, :3]) for i in range(3))


# -- the binding -------------------------------------------------------------------------------
p, i = c_void_p, c_int
NULL_CALL = (None, 1, 4, 4, 12, None, 2, 2, 8, None, None, None, None)
OVERLAY = thb.Binding(
    'overlay', 'kbe_overlay',
    # frames, n, W, H, stride; overlay, w, h, overlay stride; x, y, opacity; stream
    {'kbe_overlay_abi_version': (c_int, []), 'kbe_overlay_u8': (c_int, [p, i, i, i, i, p, i, i, i, p, p, p, p])},
    'kbe_overlay_abi_version', ['#define KBE_OVERLAY_ABI_VERSION 1\n', '#define KBE_OVERLAY_FRAMES_PER_LAUNCH 12 '],
    ['KBE_OVERLAY_BGR'], {'ABI_VERSION': 1, 'FRAMES_PER_LAUNCH': 12, 'MAX_SIDE': 65535, 'MAX_OPACITY': 256},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
     ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n'), ('kbe_dof.h', '#define KBE_DOF_ABI_VERSION 1\n'), ('kbe_shutter.h', '#define KBE_SHUTTER_ABI_VERSION 1\n'),
     ('kbe_yuv.h', '#define KBE_YUV_ABI_VERSION 1\n'), ('kbe_transition.h', '#define KBE_TRANSITION_ABI_VERSION 1\n')],
    ('kbe_overlay_u8', NULL_CALL, 'kbe_overlay_u8: null frames_u8'),
    ('kbe_overlay_u8', None, lambda frames: ((frames, 1.0, 4, 4, 12, frames, 2, 2, 8, frames, frames, frames, None), (frames, 1, 4, 4, c_size_t(12), frames, 2, 2, 8, frames, frames, frames, None),
                                             (frames, 1, 4, 4, 12, frames, 0.5, 2, 8, frames, frames, frames, None), (frames, 1, 4, 4, 12, frames, 2, 2, 8, frames, frames, frames))),
    [('kbe_overlay_abi_version', 0, (1,)), ('kbe_overlay_u8', 13, NULL_CALL + (0,)), ('kbe_overlay_u8', 13, NULL_CALL[:-1])],
    ['kbe_transition_u8', 'kbe_yuv420_u8', 'kbe_shutter_mean_u8', 'kbe_dof_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_overlay_u8', lambda at: ((c_void_p * 2)(at, at + 1024), 2, 16, 17, 48, at + 4096, 5, 5, 20, (c_int32 * 2)(0, 0), (c_int32 * 2)(0, 0), (c_int32 * 2)(256, 257), None),
     'kbe_overlay_u8 failed (-1): kbe_overlay_u8: an element of opacity outside 0..256'),
    ['kbe_overlay_u8'], set())
# what the other headers' modules declare: the lists this header must leave as they are
OTHERS = {'gif': list(thb.GIF.protos), 'area': list(thb.AREA.protos), 'crop_area': ['kbe_crop_area_abi_version', 'kbe_crop_area_u8'], 'dof': ['kbe_dof_abi_version', 'kbe_dof_u8'],
          'shutter': ['kbe_shutter_abi_version', 'kbe_shutter_mean_u8'], 'yuv': ['kbe_yuv_abi_version', 'kbe_yuv420_bytes', 'kbe_yuv420_u8'],
          'transition': ['kbe_transition_abi_version', 'kbe_transition_u8']}


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(OVERLAY)
    from ken_burns_effect_amd import overlay
    assert list(overlay.prototypes()) == ['kbe_overlay_abi_version', 'kbe_overlay_u8']


def test_the_library_exports_them_beside_the_others():
    import importlib
    thb.test_the_library_exports_them_with_the_headers_types(OVERLAY)
    from ken_burns_effect_amd import _native, overlay
    lib = overlay.load()
    assert lib is _native.load() and lib.kbe_overlay_abi_version() == 1 == overlay.ABI_VERSION
    for name, entries in OTHERS.items():
        module = importlib.import_module('ken_burns_effect_amd.' + name)
        assert module.load() is lib and getattr(lib, entries[0])() == 1


def test_the_older_headers_and_their_bindings_are_what_they_were():
    import importlib
    from ken_burns_effect_amd import _native, overlay
    b = OVERLAY
    overlay.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for name, entries in OTHERS.items():
        other = importlib.import_module('ken_burns_effect_amd.' + name)
        assert list(other.prototypes()) == entries and other.ABI_VERSION == 1
    # overlay.py is the only module of the package whose text names the header's prefix, and it names no entry of another header
    package = os.path.dirname(overlay.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and b.prefix in open(os.path.join(package, name)).read()]
    assert naming == ['overlay.py']
    with open(overlay.__file__) as f:
        text = f.read()
    foreign = set(_native.SYMBOLS) | {entry for entries in OTHERS.values() for entry in entries}
    assert not [entry for entry in sorted(foreign) if entry in text]
    name, args, text = b.null_call
    assert overlay._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(OVERLAY)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(OVERLAY)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(OVERLAY)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(OVERLAY)


def test_the_header_states_the_cut_into_launches():
    from ken_burns_effect_amd import overlay
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'kbe_overlay.hip')) as f:
        text = f.read()
    assert 'kFramesPerLaunch = KBE_OVERLAY_FRAMES_PER_LAUNCH' in text and 'asm' not in text.replace('assembl', '')
    assert overlay.FRAMES_PER_LAUNCH == 12
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'Makefile')) as f:
        text = f.read()
    assert ' kbe_overlay.hip' in text and ' kbe_overlay_block.h' in text and '../../include/kbe_overlay.h' in text


# (frames of 16 x 17 at a stride of 48: 816 bytes, at 0 and 2048 of 32 KiB of host memory; the overlay, 5 x 5 at a stride of 20: 100 bytes, at 8192)
OVERLAPS_FRAME, OVERLAPS_OVERLAY = 'an element of frames_u8 overlaps another frame', 'an element of frames_u8 overlaps the overlay'
REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null overlay': (dict(overlay_rgba=None), 'null overlay_rgba'), 'null x': (dict(x=None), 'null x'),
           'null y': (dict(y=None), 'null y'), 'null opacity': (dict(opacity=None), 'null opacity'), 'n = 0': (dict(n=0), 'n < 1'), 'n = -1': (dict(n=-1), 'n < 1'),
           'W = 0': (dict(W=0), 'W or H outside 1..65535'), 'W = 65536': (dict(W=65536, stride_bytes=3 * 65536), 'W or H outside 1..65535'),
           'H = 0': (dict(H=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'), 'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'),
           'w = 0': (dict(w=0), 'w or h outside 1..65535'), 'w = 65536': (dict(w=65536, overlay_stride_bytes=4 * 65536), 'w or h outside 1..65535'),
           'h = 0': (dict(h=0), 'w or h outside 1..65535'), 'h = 65536': (dict(h=65536), 'w or h outside 1..65535'), 'overlay stride': (dict(overlay_stride_bytes=19), 'overlay_stride_bytes < 4 w'),
           'null frame 1': (dict(frames_u8=(None, 0)), 'null element of frames_u8'),
           'x 65536': (dict(x=(0, 65536)), 'an element of x outside -65535..65535'), 'x -65536': (dict(x=(-65536, 0)), 'an element of x outside -65535..65535'),
           'y 65536': (dict(y=(65536, 0)), 'an element of y outside -65535..65535'), 'y -65536': (dict(y=(0, -65536)), 'an element of y outside -65535..65535'),
           'opacity 257': (dict(opacity=(256, 257)), 'an element of opacity outside 0..256'), 'opacity -1': (dict(opacity=(-1, 256)), 'an element of opacity outside 0..256'),
           'the same frame twice': (dict(frames_u8=(None, 1)), OVERLAPS_FRAME), 'one byte into the next frame': (dict(frames_u8=(2048 - 815 + 1, None)), OVERLAPS_FRAME),
           'the overlay is a frame': (dict(overlay_rgba=2048), OVERLAPS_OVERLAY), 'the overlay on a frames last byte': (dict(overlay_rgba=815), OVERLAPS_OVERLAY),
           'a frame on the overlays last byte': (dict(frames_u8=(None, 8192 + 99 + 1)), OVERLAPS_OVERLAY),
           # (wholly outside and at opacity 0: nothing would be launched, and the overlap is refused all the same)
           'an overlap of frames that are in no launch': (dict(frames_u8=(None, 1), x=(16, 16), opacity=(0, 0)), OVERLAPS_FRAME)}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, overlay
    memory = (ctypes.c_uint64 * 4096)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 2)(at, at + 2048), n=2, W=16, H=17, stride_bytes=48, overlay_rgba=at + 8192, w=5, h=5, overlay_stride_bytes=20,
                x=(c_int32 * 2)(1, 2), y=(c_int32 * 2)(3, 4), opacity=(c_int32 * 2)(256, 128), stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key == 'frames_u8' and isinstance(value, tuple):
            for k in (0, 1):                                                # (None: as it was; 0: null; 1: the other frame's pointer; else an offset)
                if value[k] is not None:
                    args[key][k] = None if value[k] == 0 else args[key][1 - k] if value[k] == 1 else at + value[k] - 1
        elif key in ('x', 'y', 'opacity') and value is not None:
            args[key] = (c_int32 * 2)(*value)
        elif key == 'overlay_rgba' and value is not None:
            args[key] = at + value
        else:
            args[key] = value
    assert overlay._raw('kbe_overlay_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_overlay_u8: ' + text
    assert not any(memory)


def test_apply_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, overlay
    good, picture = torch.zeros(4, 8, 8, 3, dtype=torch.uint8), torch.zeros(3, 3, 4, dtype=torch.uint8)
    for bad in (good, np.zeros((4, 8, 8, 3), np.uint8), torch.zeros(4, 8, 8, 3), torch.zeros(8, 8, 3, dtype=torch.uint8), None):
        with pytest.raises(_native.KbeError, match=r'overlay\.apply'):
            overlay.apply(bad, picture, 0, 0)


# -- where and when ----------------------------------------------------------------------------
def test_place_against_hand_written_values():
    from ken_burns_effect_amd import overlay
    want = {'top-left': (4, 4), 'top': (27, 4), 'top-right': (50, 4), 'left': (4, 21), 'centre': (27, 21), 'right': (50, 21), 'bottom-left': (4, 38), 'bottom': (27, 38),
            'bottom-right': (50, 38)}
    assert set(want) == set(overlay.ANCHORS)
    for anchor, at in want.items():
        assert overlay.place(anchor, 64, 48, 10, 6, 4) == at, anchor
    assert overlay.place('bottom-right', 1024, 1024, 200, 50, 32) == (792, 942) and overlay.place('centre', 9, 9, 4, 4, 100) == (2, 2)
    assert overlay.place('3,-5', 64, 48, 10, 6, 4) == (3, -5) and overlay.place(' 7 , 8 ', 1, 1, 1, 1, 0) == (7, 8) and overlay.place('-1,-2', 64, 48, 10, 6, 4) == (-1, -2)
    for bad in ('middle', '1,2,3', '1;2', 'x,y', '', '1.5,2', '--1,2', None, 5):
        with pytest.raises(ValueError):
            overlay.place(bad, 64, 48, 10, 6, 4)


def test_the_opacity_table_against_hand_written_values():
    from ken_burns_effect_amd import overlay
    table = overlay.opacity_table
    assert table(10, 2, 9, 2) == [0, 0, 85, 171, 256, 256, 256, 171, 85, 0]
    assert table(6, 0, 6, 3) == [64, 128, 192, 192, 128, 64] and table(5, 1, 4, 0) == [0, 256, 256, 256, 0] and table(3, 0, 0, 0) == [0, 0, 0]
    assert table(4, 0, 4, 1, 128) == [64, 128, 128, 64] and table(4, 1, 3, 1) == [0, 128, 128, 0] and table(4, 1, 3, 0, 77) == [0, 77, 77, 0]
    assert table(5, 0, 5, 2, 255) == [85, 170, 255, 170, 85]                 # (85 * 255 + 128) >> 8 = 85, (171 * 255 + 128) >> 8 = 170
    got = table(75, 12, 63, 12)
    assert len(got) == 75 and got[:12] == [0] * 12 and got[63:] == [0] * 12 and got[24:51] == [256] * 27 and got[12:24] == got[51:63][::-1] and 0 < got[12] < got[23] < 256
    for args in ((10, 2, 5, 2), (10, 2, 9, 4), (10, 5, 4, 0), (10, -1, 4, 0), (10, 0, 11, 0), (10, 0, 10, -1), (10, 0, 10, 1, 257)):
        with pytest.raises(ValueError, match=r'^overlay\.opacity_table: '):
            table(*args)


def test_the_caption_windows_against_hand_written_values():
    from ken_burns_effect_amd import slideshow
    assert slideshow.caption_windows(75, 3, 12, 5, 7) == [(5, 63), (12, 63), (12, 68)]
    assert slideshow.caption_windows(6, 2, 2) == [(0, 4), (2, 6)] and slideshow.caption_windows(6, 1, 0, 1, 2) == [(1, 4)]
    show = slideshow.checked([(64, 48), (64, 48)], 6, 'dissolve', 2, captions=['one', 'two'], caption_fade=1)
    assert show['windows'] == [(0, 4), (2, 6)] and show['captions'] == ['one', 'two'] and show['caption_fade'] == 1 and show['steps'] == 6
    # a window is the clip's frames of the plan that are the clip's own, neither a junction's nor a fade's
    for lengths, T, fi, fo in ((3, 12, 5, 7), (2, 2, 0, 0), (1, 0, 9, 3), (4, 30, 0, 45)):
        show = slideshow.checked([(64, 48)] * lengths, 75, 'wipe-left', T if lengths > 1 else 12, None, '0,0,0', fi, fo)
        own = [[q[2] for q in show['plan'] if q[0] == 'clip' and q[1] == c] for c in range(lengths)]
        assert show['windows'] == [(frames[0], frames[-1] + 1) if frames else (w[0], w[0]) for frames, w in zip(own, show['windows'])]
    captions, watermark = slideshow.show_layers(slideshow.checked([(64, 48), (64, 48)], 6, 'dissolve', 2, captions=['one', ''], caption_fade=1), None)
    assert watermark is None and captions[1] is None and captions[0][3] == [128, 256, 256, 128, 0, 0] and captions[0][0].shape[2] == 4
    assert slideshow.show_layers(slideshow.checked([(64, 48)], 6), None) == ([], None)


# -- the pictures ------------------------------------------------------------------------------
def test_the_caption_is_its_over_formula_on_pillows_mask():
    """No glyph byte is pinned: the mask is Pillow's, asked for again here; what is held is everything this package makes of it."""
    from ken_burns_effect_amd import overlay
    text, size, colour, plate = 'Hi\nthere, AMD', 20, (250, 240, 10), (10, 20, 30, 128)
    mask = overlay.caption_mask(text, size)
    assert mask.dtype == np.uint8 and mask.max() > 128 and mask.min() == 0 and 0 < (mask > 0).mean() < 0.6 and mask.shape[0] > size       # (two lines)
    picture = overlay.caption_image(text, size, colour, plate, bgr=False)
    pad = size // 2
    assert picture.shape == (mask.shape[0] + 2 * pad, mask.shape[1] + 2 * pad, 4) and picture.dtype == np.uint8
    whole = np.zeros(picture.shape[:2])
    whole[pad:-pad, pad:-pad] = mask / 255.0
    alpha_plate = plate[3] / 255.0
    alpha = whole + alpha_plate * (1.0 - whole)                              # `over`, straight alpha
    assert (np.abs(picture[:, :, 3] - 255.0 * alpha) <= 0.5 + 1e-9).all()
    for k in range(3):
        exact = (colour[k] * whole + plate[k] * alpha_plate * (1.0 - whole)) / alpha
        assert (np.abs(picture[:, :, k] - exact) <= 0.5 + 1e-9).all()
    border = np.ones(picture.shape[:2], bool)
    border[pad:-pad, pad:-pad] = False
    assert (picture[border] == plate).all() and (picture[whole == 1.0] == colour + (255,)).all() and (picture[(whole == 0.0) & ~border] == plate).all()
    swapped = overlay.caption_image(text, size, colour, plate)
    assert np.array_equal(swapped[:, :, [2, 1, 0, 3]], picture)
    # a clear plate: the text alone, its alpha the mask; an opaque one: alpha 255 everywhere
    alone = overlay.caption_image(text, size, colour, (0, 0, 0, 0), bgr=False)
    assert np.array_equal(alone[pad:-pad, pad:-pad, 3], mask) and (alone[:, :, :3][alone[:, :, 3] > 0] == colour).all() and (alone[alone[:, :, 3] == 0] == 0).all()
    assert (overlay.caption_image(text, size, colour, (1, 2, 3, 255))[:, :, 3] == 255).all()
    default = overlay.caption_image('x', 12)
    assert (default[0, 0] == (0, 0, 0, 128)).all() and default[:, :, :3].max() > 0 and default[:, :, 3].max() > 128
    for bad in (('', 12), ('  \n ', 12), ('x', 3), (None, 12)):
        with pytest.raises(ValueError):
            overlay.caption_image(*bad)
    for kw in (dict(colour=(1, 2)), dict(colour=(1, 2, 256)), dict(plate=(0, 0, 0)), dict(plate=(0, 0, 0, -1))):
        with pytest.raises(ValueError, match='colour'):
            overlay.caption_image('x', 12, **kw)


def test_read_rgba(tmp_path):
    from ken_burns_effect_amd import overlay
    rgba = np.dstack([gc.photo_like(6, 9, 3), np.arange(54, dtype=np.uint8).reshape(6, 9) * 4])
    Image.fromarray(rgba, 'RGBA').save(str(tmp_path / 'logo.png'))
    Image.fromarray(rgba[:, :, :3].copy()).save(str(tmp_path / 'plain.png'))
    assert np.array_equal(overlay.read_rgba(str(tmp_path / 'logo.png'), False), rgba) and np.array_equal(overlay.read_rgba(str(tmp_path / 'logo.png'), True), rgba[:, :, [2, 1, 0, 3]])
    plain = overlay.read_rgba(str(tmp_path / 'plain.png'), True)
    assert plain.shape == (6, 9, 4) and (plain[:, :, 3] == 255).all() and np.array_equal(plain[:, :, :3], rgba[:, :, 2::-1]) and plain.flags['C_CONTIGUOUS']
    with pytest.raises(OSError):
        overlay.read_rgba(str(tmp_path / 'none.png'), True)


# -- the command lines -------------------------------------------------------------------------
ENV = ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_JPEG', 'KBE_PNG', 'KBE_OVERLAY', 'KBE_OVERLAY_AT', 'KBE_OVERLAY_OPACITY', 'KBE_CAPTION', 'KBE_CAPTION_AT', 'KBE_CAPTION_SIZE',
       'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES', 'KBE_Y4M')
ANCHORS = 'top-left, top, top-right, left, centre, right, bottom-left, bottom, bottom-right, or X,Y'
LONG = 'a caption that is far too long to fit into a frame of sixty-four pixels'


def _pictures(tmp_path):
    paths = {}
    for name, (w, h) in (('logo', (10, 6)), ('big', (70, 10)), ('tall', (10, 45)), ('mid', (30, 8))):
        paths[name] = str(tmp_path / (name + '.png'))
        Image.fromarray(np.dstack([gc.photo_like(h, w, 2), np.full((h, w), 200, np.uint8)]), 'RGBA').save(paths[name])
    paths['text'] = str(tmp_path / 'notes.txt')
    with open(paths['text'], 'w') as f:
        f.write('not a picture')
    paths['none'] = str(tmp_path / 'none.png')
    return paths


def _kbe_refusals(P):
    fits = r'it is %s and the frames are %s: with a margin of %d it does not fit inside them$'
    return (
        (['--overlay', P['none']], r'^--overlay %s: no such file$' % re.escape(P['none'])), (['--overlay', P['text']], r'^--overlay %s: not a picture Pillow reads' % re.escape(P['text'])),
        (['--overlay', P['big']], r'^--overlay %s: ' % re.escape(P['big']) + fits % ('70x10', '64x48', 4)), (['--overlay', P['tall']], r'^--overlay .*tall\.png: ' + fits % ('10x45', '64x48', 4)),
        (['--overlay', P['mid'], '--width', '32'], r'^--overlay .*mid\.png: ' + fits % ('30x8', '32x24', 4)), (['--overlay', P['logo'], '--overlay-margin', '28'], r'^--overlay .*: ' + fits % ('10x6', '64x48', 28)),
        (['--caption', ''], r"^--caption '': an empty caption$"), (['--caption', '  '], r"^--caption '  ': an empty caption$"),
        (['--caption', LONG], r"^--caption '%s': it is \d+x\d+ and the frames are 64x48: with a margin of 4 it does not fit inside them$" % LONG),
        (['--caption', 'hi', '--caption-size', '40'], r"^--caption 'hi': it is \d+x\d+ and the frames are 64x48: "),
        (['--overlay', P['logo'], '--overlay-opacity', '0'], r'^--overlay-opacity 0: above 0 and at most 1$'), (['--overlay', P['logo'], '--overlay-opacity', '1.5'], r'^--overlay-opacity 1\.5: '),
        (['--overlay', P['logo'], '--overlay-opacity', 'half'], r'^--overlay-opacity half: '), (['--overlay', P['logo'], '--overlay-opacity', '-1'], r'^--overlay-opacity -1: '),
        (['--overlay', P['logo'], '--overlay-opacity', 'nan'], r'^--overlay-opacity nan: '), (['--overlay', P['logo'], '--overlay-opacity', '0.001'], r'^--overlay-opacity 0\.001: '),
        (['--caption', 'hi', '--caption-size', '3'], r"^--caption-size 3: the font's size in pixels, 4 or more$"), (['--caption', 'hi', '--caption-size', 'big'], r'^--caption-size big: '),
        (['--overlay-at', 'top'], r'^--overlay-at top: only with --overlay$'), (['--overlay-opacity', '0.5'], r'^--overlay-opacity 0\.5: only with --overlay$'),
        (['--caption-at', 'top'], r'^--caption-at top: only with --caption$'), (['--caption-size', '20'], r'^--caption-size 20: only with --caption$'),
        (['--font', P['none']], r'^--font .*: only with --caption$'), (['--overlay-margin', '3'], r'^--overlay-margin 3: only with --overlay or --caption$'),
        (['--caption', 'hi', '--overlay-at', '1,2'], r'^--overlay-at 1,2: only with --overlay$'), (['--overlay', P['logo'], '--caption-at', '1,2'], r'^--caption-at 1,2: only with --caption$'),
        (['--overlay', P['logo'], '--overlay-at', 'middle'], r'^--overlay-at middle: %s$' % ANCHORS), (['--caption', 'hi', '--caption-at', '1,2,3'], r'^--caption-at 1,2,3: %s$' % ANCHORS),
        (['--caption', 'hi', '--font', P['none']], r'^--font %s: no such file$' % re.escape(P['none'])), (['--caption', 'hi', '--font', P['text']], r'^--font %s: ' % re.escape(P['text'])),
        (['--overlay', P['logo'], '--overlay-margin', '-1'], r'^--overlay-margin -1: pixels, 0 or more$'), (['--overlay', P['logo'], '--overlay-margin', 'wide'], r'^--overlay-margin wide: '))


def test_kbe_refuses_before_a_network_is_built(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import kbe, overlay, pipeline
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    built = []

    class Stop(Exception):
        pass

    def init(self, *a, **k):
        built.append(k)
        raise Stop()
    monkeypatch.setattr(pipeline.Pipeline, '__init__', init)
    P = _pictures(tmp_path)
    photo, out = str(tmp_path / 'in.png'), str(tmp_path / 'out')
    Image.fromarray(gc.photo_like(48, 64, 1)).save(photo)
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        for argv, text in _kbe_refusals(P):
            with pytest.raises(SystemExit, match=text):
                kbe.main(['--in', photo, '--out', out] + argv)
        assert built == [] and not os.path.exists(out)
        # what is in order reaches the Pipeline, as it was given; an explicit position needs no fit
        for argv in (['--overlay', P['logo'], '--overlay-at', 'top-left', '--overlay-opacity', '0.5', '--caption', 'hi\nyou', '--caption-at', '2,3', '--caption-size', '12', '--overlay-margin', '2'],
                     ['--overlay', P['big'], '--overlay-at', '-3,40'], ['--overlay', P['mid'], '--width', '48'], []):
            with pytest.raises(Stop):
                kbe.main(['--in', photo, '--out', out] + argv)
        # the environment's twins
        monkeypatch.setenv('KBE_CAPTION', '')
        monkeypatch.setenv('KBE_OVERLAY', P['big'])
        with pytest.raises(SystemExit, match=r'^--overlay .*big\.png: it is 70x10'):
            kbe.main(['--in', photo, '--out', out])
        monkeypatch.setenv('KBE_OVERLAY_AT', '0,0')
        monkeypatch.setenv('KBE_OVERLAY_OPACITY', '0.25')
        monkeypatch.setenv('KBE_CAPTION', 'from the environment')
        monkeypatch.setenv('KBE_CAPTION_AT', 'top')
        monkeypatch.setenv('KBE_CAPTION_SIZE', '9')
        request = kbe.parse([])[0]['layers']
        assert request == dict(overlay=P['big'], overlay_at='0,0', overlay_opacity=64, caption='from the environment', caption_at='top', caption_size=9, font=None, overlay_margin=None)
        assert kbe.parse(['--caption', 'mine', '--overlay-opacity', '1'])[0]['layers']['caption'] == 'mine' and kbe.parse(['--overlay-opacity', '1'])[0]['layers']['overlay_opacity'] == 256
    finally:
        torch.set_grad_enabled(grad)
    assert len(built) == 4 and not os.path.exists(out)
    assert built[0]['overlay'] == P['logo'] and built[0]['overlay_at'] == 'top-left' and built[0]['overlay_opacity'] == '0.5' and built[0]['caption'] == 'hi\nyou'
    assert built[0]['caption_at'] == '2,3' and built[0]['caption_size'] == '12' and built[0]['overlay_margin'] == '2' and built[0]['font'] is None
    assert all(built[3][name] is None for name in overlay.OPTIONS) and set(overlay.OPTIONS) <= set(built[3])
    # the defaults, and the layers of a request, in their order: the caption first
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    assert overlay.layers_request() is None and pipeline.layers_of(type('Bare', (), {})(), (64, 48)) == [] and pipeline.layers_of(type('Bare', (), {})(), lambda: 1 / 0) == []
    layers = overlay.layers_for(overlay.layers_request(overlay=P['logo'], caption='hi'), 1024, 512)
    assert [(x, y, opacity) for _, x, y, opacity in layers] == [((1024 - layers[0][0].shape[1]) // 2, 512 - layers[0][0].shape[0] - 32, 256), (1024 - 10 - 32, 512 - 6 - 32, 256)]
    assert layers[0][0].shape[0] == overlay.caption_image('hi', 512 // 18).shape[0] and np.array_equal(layers[1][0], overlay.read_rgba(P['logo'], True))
    assert '--overlay FILE' in kbe.__doc__ and '--caption TEXT' in kbe.__doc__ and 'KBE_CAPTION_SIZE' in kbe.__doc__


def test_the_slideshow_refuses_before_a_network_is_built(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import pipeline, slideshow
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    built = []

    class Stop(Exception):
        pass

    def init(self, *a, **k):
        built.append(k)
        raise Stop()
    monkeypatch.setattr(pipeline.Pipeline, '__init__', init)
    P = _pictures(tmp_path)
    photos, out = [str(tmp_path / ('in%d.png' % k)) for k in range(2)], str(tmp_path / 'out')
    for k, path in enumerate(photos):
        Image.fromarray(gc.photo_like(48, 64, 1 + k)).save(path)
    refusals = (
        (2, ['--caption', 'one'], r'^--caption: 1 captions for 2 photos: one per photo'), (1, ['--caption', 'one', '--caption', 'two'], r'^--caption: 2 captions for 1 photos: '),
        (2, ['--caption', 'a', '--caption', 'b', '--caption-fade', '32'], r'^--caption-fade 32: 0\.\.31, half of the 63 frames of a captioned clip that no transition or fade uses$'),
        (2, ['--caption-fade', 'slow'], r'^--caption-fade slow: '), (2, ['--caption', '', '--caption', 'b', '--fade-out', '60', '--caption-fade', '2'], r'^--caption-fade 2: 0\.\.1, half of the 3 frames'),
        (1, ['--caption', 'a', '--fade-in', '40', '--fade-out', '30', '--caption-fade', '3'], r'^--caption-fade 3: 0\.\.2, half of the 5 frames'),
        (2, ['--caption-at', 'top'], r'^--caption-at top: only with --caption$'), (2, ['--caption', '', '--caption', '', '--caption-at', 'top'], r'^--caption-at top: only with --caption$'),
        (2, ['--caption', 'a', '--caption', LONG], r"^--caption '%s': it is \d+x\d+ and the frames are 64x48: " % LONG), (2, ['--overlay', P['big']], r'^--overlay .*big\.png: it is 70x10 and the frames are 64x48'),
        (2, ['--overlay', P['mid'], '--width', '32'], r'^--overlay .*mid\.png: it is 30x8 and the frames are 32x24'), (1, ['--overlay', P['none']], r'^--overlay .*: no such file$'),
        (1, ['--overlay', P['logo'], '--overlay-opacity', '2'], r'^--overlay-opacity 2: '), (1, ['--caption', 'a', '--caption-size', '2'], r'^--caption-size 2: '))
    grad = torch.is_grad_enabled()
    try:
        for count, argv, text in refusals:
            with pytest.raises(SystemExit, match=text):
                slideshow.main([v for path in photos[:count] for v in ('--in', path)] + ['--out', out] + argv)
        assert built == [] and not os.path.exists(out)
        for argv in (['--caption', 'one', '--caption', '', '--overlay', P['logo'], '--caption-fade', '31', '--caption-at', 'top'],
                     ['--caption', '', '--caption', '', '--caption-fade', '99'], ['--caption', '', '--caption', 'b', '--fade-out', '60', '--caption-fade', '1']):
            with pytest.raises(Stop):
                slideshow.main(['--in', photos[0], '--in', photos[1], '--out', out] + argv)
    finally:
        torch.set_grad_enabled(grad)
    # the slideshow's Pipeline is built without either layer
    assert len(built) == 3 and not os.path.exists(out) and all('overlay' not in k and 'caption' not in k for k in built)
    cfg = slideshow.parse(['--in', 'a', '--in', 'b', '--caption', 'x', '--caption', '', '--overlay', P['logo']])
    assert cfg['caption'] == ['x', ''] and cfg['caption-fade'] == '12' and cfg['layers']['overlay'] == P['logo'] and cfg['layers']['caption_at'] == 'bottom'
    assert slideshow.parse(['--in', 'a'])['layers'] is None and slideshow.parse(['--in', 'a'])['caption'] == []
    assert 'caption-fade=' in slideshow.LONG_OPTIONS and 'caption=' in slideshow.LONG_OPTIONS and '--caption-fade F' in slideshow.__doc__
