"""The transitions (include/kbe_transition.h) without a GPU: csrc/kbe_transition_block.h executed serially (tests/transition_check.cpp) against the
plain definition and against the NumPy twin (tests/transition_cases.py); the pinned values; the binding (transition.py) held to what
tests/test_header_bindings.py holds the older headers to; every refusal of the entry on host memory; transition.join's layout; and the
slideshow command line's refusals."""
import ctypes
import inspect
import os
import re
from ctypes import c_int, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest
from PIL import Image

import gif_cases as gc
import test_header_bindings as thb
import transition_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition ---------------------------------------------------------------------------
def test_the_packed_forms_are_the_plain_one():
    """transition_check.cpp builds; all 256 x 256 x 257 blends, packed against plain; the wipes' weight by the multiply-high against the plain
    division for every p in 0..256, eight extents L from 1 to 65535, nine softnesses s from 1 to 65535 and every t (and six places either side of the row); x = j / 3 for every j; the colour dwords;
    whole frames of every kind, lane by lane at all 256 pairs of alignment classes.  All mismatch counts are zero."""
    m = re.search(r'brute: blends (\d+), plain mismatches (\d+), packed mismatches (\d+), weights (\d+), weight mismatches (\d+), thirds (\d+), third mismatches (\d+), '
                  r'colour mismatches (\d+), frames (\d+), frame mismatches (\d+)', tc.ask('brute'))
    blends, plain, packed, weights, weight_bad, thirds, third_bad, colour_bad, frames, frame_bad = (int(v) for v in m.groups())
    assert blends == 256 * 256 * 257 and weights == 257 * 9 * sum(L + 12 for L in (1, 2, 5, 50, 341, 400, 1366, 65535))
    assert thirds >= 2 * 3 * 65535 and frames == 6 * 6 * 256
    assert (plain, packed, weight_bad, third_bad, colour_bad, frame_bad) == (0,) * 6


def _flat(v):
    return np.full((1, 3, 5, 3), v, np.uint8)


def test_the_pinned_values():
    """The pinned values of blend, for the twin, and for the header through a dissolve of flat frames at p = w."""
    pinned = (((0, 255, 128), 128), ((255, 0, 128), 128), ((0, 255, 1), 1), ((0, 255, 255), 254), ((10, 20, 64), 13))
    for (a, b, w), want in pinned:
        assert tc.blend(a, b, w) == want
        for blend in (tc.twin_blend, tc.header_blend):
            assert (blend(_flat(a), _flat(b), 'dissolve', [w]) == want).all(), (a, b, w, blend.__name__)
    v, w = np.meshgrid(np.arange(256), np.arange(257))
    assert np.array_equal(tc.blend(v, v, w), v)
    assert int(tc.blend(255, 255, 128)) == 255 and 255 * 256 + 128 == 65408 < 1 << 16


def test_the_pinned_wipe():
    """W = 50, s = 8, p = 128: w = 256 for x <= 21, 0 for x >= 29, and 224, 192, ..., 32 in between; for the twin and for the header's lanes."""
    want = [256] * 22 + [224, 192, 160, 128, 96, 64, 32] + [0] * 21
    for weights in (tc.weight_map, tc.header_weights):
        assert weights('wipe-right', 128, 50, 3, 8).tolist() == [want] * 3, weights.__name__
        assert weights('wipe-left', 128, 50, 3, 8).tolist() == [want[::-1]] * 3
        assert weights('wipe-down', 128, 3, 50, 8).T.tolist() == [want] * 3
        assert weights('wipe-up', 128, 3, 50, 8).T.tolist() == [want[::-1]] * 3


def test_the_progress_table():
    from ken_burns_effect_amd import transition
    for table in (tc.progress_table, transition.progress_table):
        assert table(1) == [128] and table(2) == [85, 171] and table(3) == [64, 128, 192] and table(0) == []
        for T in range(1, 200):
            got = table(T)
            assert len(got) == T and got == sorted(got) and 0 < got[0] and got[-1] < 256
            assert all(abs(2 * (T + 1) * p - 512 * (j + 1)) <= T + 1 for j, p in enumerate(got))           # within 1/2 of 256 (j + 1) / (T + 1)
    assert transition.KINDS == tc.KINDS == {'dissolve': 0, 'wipe-right': 1, 'wipe-left': 2, 'wipe-down': 3, 'wipe-up': 4, 'fade': 5}


@pytest.mark.parametrize('kind', sorted(tc.KINDS))
@pytest.mark.parametrize('frame', tc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_header_is_the_twin(frame, kind):
    """blend_row of csrc/kbe_transition_block.h on the GPU suite's frames, source rows padded by 5 (every row at another alignment): the NumPy
    twin byte for byte, on inputs that tell: the dissolve differs from both sources in more than half of its bytes, a wipe's weights hold 0,
    256 and s - 1 values between, and the fade's colour bytes permuted give another frame."""
    W, H = frame
    a, b = tc.frames_of(W, H)
    want = tc.twin_of(W, H, kind)
    assert np.array_equal(tc.header_blend(a, b, kind, tc.PROGRESS, tc.SOFTNESS, tc.COLOUR, pad=5), want)
    if kind == 'dissolve':
        assert (want[0] != a[0]).mean() > 0.5 and (want[0] != b[0]).mean() > 0.5
    elif kind == 'fade':
        permuted = 200 | (90 << 8) | (10 << 16)
        assert (tc.twin_blend(a, b, kind, tc.PROGRESS, tc.SOFTNESS, permuted) != want).mean() > 0.5
    else:
        values = set(np.unique(tc.weight_map(kind, 128, W, H, tc.SOFTNESS)).tolist())
        assert {0, 256} <= values and len(values - {0, 256}) >= tc.SOFTNESS - 1
        assert np.array_equal(tc.header_weights(kind, 128, W, H, tc.SOFTNESS), tc.weight_map(kind, 128, W, H, tc.SOFTNESS))


@pytest.mark.parametrize('kind', sorted(tc.KINDS))
def test_the_endpoints_and_equal_sources(kind):
    """p = 0 gives `from` and p = 256 gives `to`, byte for byte; from == to gives that frame under the dissolve and every wipe."""
    W, H = 37, 20
    a, b = tc.frames_of(W, H, 1)
    for blend in (tc.twin_blend, tc.header_blend):
        for s in (1, 8, 3 * W):
            assert np.array_equal(blend(a, b, kind, [0], s, tc.COLOUR), a) and np.array_equal(blend(a, b, kind, [256], s, tc.COLOUR), b), (blend.__name__, s)
            if kind != 'fade':
                for p in (1, 77, 128, 255):
                    assert np.array_equal(blend(a, a, kind, [p], s, tc.COLOUR), a)
    if kind == 'fade':                                                      # p = 128: the colour, and nothing of either source
        flat = np.broadcast_to(np.array([10, 200, 90], np.uint8), a.shape)
        assert np.array_equal(tc.twin_blend(a, b, kind, [128], 1, tc.COLOUR), flat) and np.array_equal(tc.header_blend(a, b, kind, [128], 1, tc.COLOUR), flat)


# -- the binding -------------------------------------------------------------------------------
p, i, u = c_void_p, c_int, c_uint32
NULL_CALL = (None, None, 1, 4, 4, 12, 0, None, 1, 0, None, 12, None)
TRANSITION = thb.Binding(
    'transition', 'kbe_transition',
    # from, to, n, W, H, stride; kind, progress, softness, colour; out, out stride; stream
    {'kbe_transition_abi_version': (c_int, []), 'kbe_transition_u8': (c_int, [p, p, i, i, i, i, i, p, i, u, p, i, p])},
    'kbe_transition_abi_version', ['#define KBE_TRANSITION_ABI_VERSION 1\n', '#define KBE_TRANSITION_DISSOLVE 0\n', '#define KBE_TRANSITION_FADE 5\n', '#define KBE_TRANSITION_FRAMES_PER_LAUNCH 12 '],
    ['KBE_TRANSITION_BGR'], {'ABI_VERSION': 1, 'FRAMES_PER_LAUNCH': 12, 'MAX_SOFTNESS': 65535, 'MAX_SIDE': 65535, 'FADE': 5},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
     ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n'), ('kbe_dof.h', '#define KBE_DOF_ABI_VERSION 1\n'), ('kbe_shutter.h', '#define KBE_SHUTTER_ABI_VERSION 1\n'),
     ('kbe_yuv.h', '#define KBE_YUV_ABI_VERSION 1\n')],
    ('kbe_transition_u8', NULL_CALL, 'kbe_transition_u8: null from_u8'),
    ('kbe_transition_u8', None, lambda frames: ((frames, frames, 1.0, 4, 4, 12, 0, frames, 1, 0, frames, 12, None), (frames, frames, 1, 4, 4, 12, 0, frames, 1, 0, frames, c_size_t(12), None),
                                                (frames, frames, 1, 4, 4, 12, 0, frames, 1, 0.5, frames, 12, None), (frames, frames, 1, 4, 4, 12, 0, frames, 1, 0, frames, 12))),
    [('kbe_transition_abi_version', 0, (1,)), ('kbe_transition_u8', 13, NULL_CALL + (0,)), ('kbe_transition_u8', 13, NULL_CALL[:-1])],
    ['kbe_yuv420_u8', 'kbe_shutter_mean_u8', 'kbe_dof_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_transition_u8', lambda at: ((c_void_p * 2)(at, at + 1024), (c_void_p * 2)(at + 2048, at + 3072), 2, 16, 17, 48, 6, (ctypes.c_int32 * 2)(1, 2), 1, 0,
                                      (c_void_p * 2)(at + 4096, at + 6144), 48, None),
     'kbe_transition_u8 failed (-1): kbe_transition_u8: kind outside 0..5'),
    ['kbe_transition_u8'], set())
# what the other headers' modules declare: the lists this header must leave as they are
OTHERS = {'gif': list(thb.GIF.protos), 'area': list(thb.AREA.protos), 'crop_area': ['kbe_crop_area_abi_version', 'kbe_crop_area_u8'], 'dof': ['kbe_dof_abi_version', 'kbe_dof_u8'],
          'shutter': ['kbe_shutter_abi_version', 'kbe_shutter_mean_u8'], 'yuv': ['kbe_yuv_abi_version', 'kbe_yuv420_bytes', 'kbe_yuv420_u8']}


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(TRANSITION)
    from ken_burns_effect_amd import transition
    assert list(transition.prototypes()) == ['kbe_transition_abi_version', 'kbe_transition_u8']


def test_the_library_exports_them_beside_the_others():
    import importlib
    thb.test_the_library_exports_them_with_the_headers_types(TRANSITION)
    from ken_burns_effect_amd import _native, transition
    lib = transition.load()
    assert lib is _native.load() and lib.kbe_transition_abi_version() == 1 == transition.ABI_VERSION
    for name, entries in OTHERS.items():
        module = importlib.import_module('ken_burns_effect_amd.' + name)
        assert module.load() is lib and getattr(lib, entries[0])() == 1


def test_the_older_headers_and_their_bindings_are_what_they_were():
    import importlib
    from ken_burns_effect_amd import _native, transition
    b = TRANSITION
    transition.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for name, entries in OTHERS.items():
        other = importlib.import_module('ken_burns_effect_amd.' + name)
        assert list(other.prototypes()) == entries and other.ABI_VERSION == 1
    # transition.py is the only module of the package whose text names the header's prefix, and it names no entry of another header
    package = os.path.dirname(transition.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and b.prefix in open(os.path.join(package, name)).read()]
    assert naming == ['transition.py']
    with open(transition.__file__) as f:
        text = f.read()
    foreign = set(_native.SYMBOLS) | {entry for entries in OTHERS.values() for entry in entries}
    assert not [entry for entry in sorted(foreign) if entry in text]
    name, args, text = b.null_call
    assert transition._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(TRANSITION)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(TRANSITION)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(TRANSITION)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(TRANSITION)


def test_the_header_states_the_cut_into_launches():
    from ken_burns_effect_amd import transition
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'kbe_transition.hip')) as f:
        assert 'kFramesPerLaunch = KBE_TRANSITION_FRAMES_PER_LAUNCH' in f.read()
    assert transition.FRAMES_PER_LAUNCH == 12


# (frames of 16 x 17 at a stride of 48: 816 bytes.  The two `from` frames lie at 0 and 2048 of 32 KiB of host memory, the two `to` frames at
# 4096 and 6144, the two outputs at 10240 and 12288; (a, b): outputs moved there, None: as it was)
OVERLAPS_SOURCE, OVERLAPS_OUTPUT = 'an element of out_u8 overlaps a source frame', 'an element of out_u8 overlaps another output'
REFUSED = {'null from': (dict(from_u8=None), 'null from_u8'), 'null to': (dict(to_u8=None), 'null to_u8'), 'null out': (dict(out_u8=None), 'null out_u8'),
           'null progress': (dict(progress=None), 'null progress'), 'n = 0': (dict(n=0), 'n < 1'), 'n = -1': (dict(n=-1), 'n < 1'),
           'W = 0': (dict(W=0), 'W or H outside 1..65535'), 'W = 65536': (dict(W=65536, stride_bytes=3 * 65536, out_stride_bytes=3 * 65536), 'W or H outside 1..65535'),
           'H = 0': (dict(H=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'),
           'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'), 'out stride': (dict(out_stride_bytes=47), 'out_stride_bytes < 3 W'),
           'kind -1': (dict(kind=-1), 'kind outside 0..5'), 'kind 6': (dict(kind=6), 'kind outside 0..5'),
           'softness 0': (dict(softness=0), 'softness outside 1..65535'), 'softness 65536': (dict(softness=65536), 'softness outside 1..65535'),
           'softness 0 under a dissolve': (dict(softness=0, kind=0), 'softness outside 1..65535'),
           'colour bit 24': (dict(colour=1 << 24), 'colour with bits 24..31 set'), 'colour bit 31': (dict(colour=1 << 31), 'colour with bits 24..31 set'),
           'null from 1': (dict(from_u8=1), 'null element of from_u8'), 'null to 0': (dict(to_u8=0), 'null element of to_u8'), 'null output 1': (dict(out_u8=1), 'null element of out_u8'),
           'progress 257': (dict(progress=(128, 257)), 'an element of progress outside 0..256'), 'progress -1': (dict(progress=(-1, 128)), 'an element of progress outside 0..256'),
           'in place': (dict(out_u8=(0, None)), OVERLAPS_SOURCE), 'output is a to frame': (dict(out_u8=(None, 4096)), OVERLAPS_SOURCE),
           'onto the other frames source': (dict(out_u8=(2048, None)), OVERLAPS_SOURCE),
           'one byte into the next from frame': (dict(out_u8=(2048 - 815, None)), OVERLAPS_SOURCE),
           'one byte into a to frame': (dict(out_u8=(None, 4096 - 815)), OVERLAPS_SOURCE),
           'the last byte of the last source': (dict(out_u8=(None, 6144 + 815)), OVERLAPS_SOURCE),
           'one outputs last byte on the others first': (dict(out_u8=(12288 - 815, None)), OVERLAPS_OUTPUT),
           'the same output twice': (dict(out_u8=(None, 10240)), OVERLAPS_OUTPUT),
           # from == to and repeated sources pass every check of the sources: the refusal is the last check's
           'equal sources': (dict(repeat=True, out_u8=(None, 10240 + 815)), OVERLAPS_OUTPUT)}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, transition
    memory = (ctypes.c_uint64 * 4096)()
    at = ctypes.addressof(memory)
    args = dict(from_u8=(c_void_p * 2)(at, at + 2048), to_u8=(c_void_p * 2)(at + 4096, at + 6144), n=2, W=16, H=17, stride_bytes=48, kind=1,
                progress=(ctypes.c_int32 * 2)(128, 64), softness=2, colour=0x123456, out_u8=(c_void_p * 2)(at + 10240, at + 12288), out_stride_bytes=48, stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key == 'repeat':
            args['from_u8'] = args['to_u8'] = (c_void_p * 2)(at, at)
        elif key in ('from_u8', 'to_u8', 'out_u8') and isinstance(value, int):
            args[key][value] = None
        elif key == 'out_u8' and isinstance(value, tuple):
            for k in (0, 1):
                if value[k] is not None:
                    args[key][k] = at + value[k]
        elif key == 'progress' and value is not None:
            args[key] = (ctypes.c_int32 * 2)(*value)
        else:
            args[key] = value
    assert transition._raw('kbe_transition_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_transition_u8: ' + text
    assert not any(memory)


def test_blend_and_join_refuse_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, transition
    good = torch.zeros(4, 8, 8, 3, dtype=torch.uint8)
    for bad in (good, np.zeros((4, 8, 8, 3), np.uint8), torch.zeros(4, 8, 8, 3), torch.zeros(8, 8, 3, dtype=torch.uint8), None):
        with pytest.raises(_native.KbeError, match=r'transition\.blend'):
            transition.blend(bad, bad, 'dissolve', [128] * 4)
        with pytest.raises(_native.KbeError, match=r'transition\.join'):
            transition.join([bad], 'dissolve', 1)
    with pytest.raises(_native.KbeError, match=r'transition\.join: no clip'):
        transition.join([], 'dissolve', 1)
    assert inspect.signature(transition.blend).parameters['out'].default is None
    assert [transition.default_softness(k, 400, 80) for k in sorted(tc.KINDS)] == [50, 50, 10, 50, 50, 10] and transition.default_softness('wipe-up', 5, 5) == 1
    assert transition.colour_of((10, 200, 90)) == tc.COLOUR == transition.colour_of(tc.COLOUR)
    for bad in (-1, 1 << 24, (1, 2), (1, 2, 256), 'red', None, 1.5):
        with pytest.raises(ValueError, match='colour'):
            transition.colour_of(bad)


# -- join's layout -----------------------------------------------------------------------------
def test_the_plan_of_a_join():
    from ken_burns_effect_amd import transition
    plan = transition.join_plan
    assert plan([5], 2) == [('clip', 0, j) for j in range(5)] == plan([5], 0) == plan([5], 99)         # (one clip: T is not looked at)
    assert plan([6, 4, 6], 2) == [('clip', 0, 0), ('clip', 0, 1), ('clip', 0, 2), ('clip', 0, 3), ('junction', 0, 1, 4, 0, 85), ('junction', 0, 1, 5, 1, 171),
                                  ('junction', 1, 2, 2, 0, 85), ('junction', 1, 2, 3, 1, 171), ('clip', 2, 2), ('clip', 2, 3), ('clip', 2, 4), ('clip', 2, 5)]
    for lengths, T in (([6, 4, 6], 1), ([6, 6], 3), ([75, 75, 75], 12), ([9, 2, 30, 7], 1)):
        got = plan(lengths, T)
        assert len(got) == sum(lengths) - (len(lengths) - 1) * T
        used = [(q[1], q[2]) for q in got if q[0] == 'clip'] + [(q[1], q[3]) for q in got if q[0] == 'junction'] + [(q[2], q[4]) for q in got if q[0] == 'junction']
        assert sorted(used) == [(c, j) for c, n in enumerate(lengths) for j in range(n)]                  # every frame of every clip is used exactly once
    # the fades: the show's first / last frames, from and to the colour
    assert plan([6], 0, fade_in=2, fade_out=3) == [('fade-in', 0, 0, 128 + 85 // 2), ('fade-in', 0, 1, 128 + 171 // 2), ('clip', 0, 2),
                                                   ('fade-out', 0, 3, 64 // 2), ('fade-out', 0, 4, 128 // 2), ('fade-out', 0, 5, 192 // 2)]
    got = plan([6, 4, 6], 2, fade_in=4, fade_out=4)
    assert [q[0] for q in got] == ['fade-in'] * 4 + ['junction'] * 4 + ['fade-out'] * 4 and got[0] == ('fade-in', 0, 0, 128 + 51 // 2) and got[-1] == ('fade-out', 2, 5, 205 // 2)
    assert all(128 < q[3] < 256 for q in got[:4]) and all(0 < q[3] < 128 for q in got[-4:])
    for lengths, T, kw, text in (([6, 4, 6], 2, dict(fade_in=5), 'fade_in = 5: 0..4'), ([6, 4, 6], 2, dict(fade_out=5), 'fade_out = 5: 0..4'), ([6, 4, 6], 3, {}, r'T = 3: 1\.\.2'),
                                 ([6, 4, 6], 0, {}, r'T = 0: 1\.\.2'), ([6], 0, dict(fade_in=4, fade_out=3), r'fade_in \+ fade_out = 7'), ([6], 0, dict(fade_in=7), 'fade_in = 7: 0..6'),
                                 ([6], 0, dict(fade_out=-1), 'fade_out = -1'), ([], 1, {}, r'\[\]: one clip or more'), ([4, 0], 1, {}, r'\[4, 0\]: one clip or more')):
        with pytest.raises(ValueError, match=r'^transition\.join: ' + text):
            plan(lengths, T, **kw)


# -- the command line --------------------------------------------------------------------------
CLI_REFUSALS = (
    (1, ['--transition', 'iris'], r'^--transition iris: dissolve, wipe-right, wipe-left, wipe-down, wipe-up, fade$'),
    (2, ['--transition-frames', '0'], r"^--transition-frames 0: 1\.\.37, half of a clip's 75 frames$"),
    (2, ['--transition-frames', '38'], r'^--transition-frames 38: 1\.\.37'), (3, ['--transition-frames', 'many'], r'^--transition-frames many: 1\.\.37'),
    (1, ['--softness', '0'], r"^--softness 0: the wipes' soft edge in pixels, 1\.\.65535$"), (2, ['--softness', '65536'], r'^--softness 65536: '), (2, ['--softness', 'soft'], r'^--softness soft: '),
    (2, ['--fade-colour', '1,2'], r'^--fade-colour 1,2: the fade colour \(--fade-colour\): R,G,B, three whole numbers 0\.\.255$'), (1, ['--fade-colour', '1,2,256'], r'^--fade-colour 1,2,256: '),
    (1, ['--fade-colour', 'red'], r'^--fade-colour red: '), (1, ['--fade-colour', '1,,3'], r'^--fade-colour 1,,3: '),
    (2, ['--fade-in', '64'], r'^--fade-in 64: 0\.\.63, the frames of a clip of 75 that no transition uses$'), (2, ['--fade-out', '70', '--transition-frames', '6'], r'^--fade-out 70: 0\.\.69'),
    (1, ['--fade-in', '76'], r'^--fade-in 76: 0\.\.75'), (1, ['--fade-in', '40', '--fade-out', '40'], r"^--fade-out 40: with --fade-in 40 more than the clip's 75 frames$"),
    (2, ['--fade-in', '-1'], r'^--fade-in -1: '), (2, ['--width', '65'], r'^--width 65: .*in0\.png: the crop is 57 pixels wide'),
    (2, ['--startU', '3'], r'^option --startU not recognized: window options are not taken'), (2, ['--gif', '--gif-width', '65'], r'^--gif-width 65: the frames are 64 pixels wide'),
    (0, [], r'^--in: a slideshow takes one photo or more$'))


def test_the_command_line_refuses_before_a_network_is_built(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import pipeline, slideshow
    for name in ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_JPEG', 'KBE_PNG'):
        monkeypatch.delenv(name, raising=False)
    built = []

    class Stop(Exception):
        pass

    def init(self, *a, **k):
        built.append(k)
        raise Stop()
    monkeypatch.setattr(pipeline.Pipeline, '__init__', init)
    paths = []
    for k, (W, H) in enumerate(((64, 48), (64, 48), (64, 48), (96, 64), (48, 64), (128, 96))):
        paths.append(str(tmp_path / ('in%d.png' % k)))
        Image.fromarray(gc.photo_like(H, W, 1 + k)).save(paths[-1])
    out = str(tmp_path / 'out')
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        for photos, argv, text in CLI_REFUSALS:
            with pytest.raises(SystemExit, match=text):
                slideshow.main([v for path in paths[:photos] for v in ('--in', path)] + ['--out', out] + argv)
        # photos whose frames differ in size: the first that differs, and both sizes
        with pytest.raises(SystemExit, match=r"^--in %s: its frames are 96x64 and %s's are 64x48: a slideshow's photos give frames of one size" % (re.escape(paths[3]), re.escape(paths[0]))):
            slideshow.main(['--in', paths[0], '--in', paths[1], '--in', paths[3], '--in', paths[4], '--out', out])
        with pytest.raises(SystemExit, match=r"^--in %s: its frames are 32x43 and %s's are 32x24" % (re.escape(paths[4]), re.escape(paths[0]))):
            slideshow.main(['--in', paths[0], '--in', paths[4], '--out', out, '--width', '32'])
        assert built == [] and not os.path.exists(out)
        # what is in order reaches the one Pipeline: 64 x 48 and 128 x 96 photos both give 48 x 36 frames at --width 48; one photo takes any T
        for argv in (['--in', paths[0], '--in', paths[5], '--width', '48', '--transition', 'wipe-left', '--fade-in', '63', '--fade-out', '63', '--fade-colour', '1,2,3'],
                     ['--in', paths[0], '--transition-frames', '99', '--fade-in', '40', '--fade-out', '35', '--softness', '65535']):
            with pytest.raises(Stop):
                slideshow.main(argv + ['--out', out])
    finally:
        torch.set_grad_enabled(grad)
    assert len(built) == 2 and built[0]['width'] == 48 and built[0]['steps'] == 75 == slideshow.STEPS and not os.path.exists(out)


def test_checked_describes_the_show():
    from ken_burns_effect_amd import slideshow
    show = slideshow.checked([(64, 48), (64, 48)], 6, 'wipe-down', 2, None, '7,8,9', 1, 2)
    assert show['size'] == (64, 48) and show['kind'] == 3 and show['T'] == 2 and show['softness'] == 6 and show['colour'] == (7, 8, 9) and len(show['plan']) == 10
    assert [q[0] for q in show['plan']] == ['fade-in'] + ['clip'] * 3 + ['junction'] * 2 + ['clip'] * 2 + ['fade-out'] * 2
    assert slideshow.checked([(64, 48)], 6, 'wipe-right', 'x', 9)['softness'] == 9 and slideshow.checked([(64, 48)], 6)['T'] == 0
    assert slideshow.checked([(400, 80), (400, 80)], 6, 'wipe-left', 3)['softness'] == 50
    assert slideshow.colour_bytes('0,0,0') == (0, 0, 0) and slideshow.colour_bytes((255, 1, 2)) == (255, 1, 2) and slideshow.colour_bytes(' 1, 2 ,3') == (1, 2, 3)
    assert 'startU=' not in slideshow.LONG_OPTIONS and 'transition=' in slideshow.LONG_OPTIONS and 'y4m' in slideshow.LONG_OPTIONS and '--fade-in N' in slideshow.__doc__


def test_write_gif_takes_back_and_render_exists():
    from ken_burns_effect_amd import gif, pipeline, yuv
    assert inspect.signature(gif.write_gif).parameters['back'].default is True and inspect.signature(gif.write_gif).parameters['back'].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(yuv.write_y4m).parameters['back'].default is True
    render = inspect.signature(pipeline.Pipeline.render).parameters
    assert list(render) == ['self', 'tensorImage', 'zoom_settings', 'bgr', 'layers'] and render['bgr'].default is True and render['layers'].default is True
