"""The binding of the colour grade (include/kbe_grade.h, ken-burns-effect_amd/grade.py) without a GPU, held to what
tests/test_header_bindings.py holds the older headers to: the header parses to exactly its two entries, the built library exports them with
the header's types, kbe.h and the other headers are what they were, grade.py is the only module that names the entries, and a wrong, a
surplus or a missing argument is refused before the call."""
import importlib
import os
from ctypes import c_int, c_int32, c_size_t, c_void_p

import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p, i = c_void_p, c_int
NULL_CALL = (None, 1, 4, 4, 12, None, 2, None, None)
GRADE = thb.Binding(
    'grade', 'kbe_grade',
    # frames, n, W, H, stride; lut, N; strength; stream
    {'kbe_grade_abi_version': (c_int, []), 'kbe_grade_u8': (c_int, [p, i, i, i, i, p, i, p, p])},
    'kbe_grade_abi_version', ['#define KBE_GRADE_ABI_VERSION 1\n', '#define KBE_GRADE_FRAMES_PER_LAUNCH 12 '],
    ['KBE_GRADE_BGR'], {'ABI_VERSION': 1, 'FRAMES_PER_LAUNCH': 12, 'MAX_SIDE': 65535, 'MAX_STRENGTH': 256, 'MIN_NODES': 2, 'MAX_NODES': 33},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
     ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n'), ('kbe_dof.h', '#define KBE_DOF_ABI_VERSION 1\n'), ('kbe_shutter.h', '#define KBE_SHUTTER_ABI_VERSION 1\n'),
     ('kbe_yuv.h', '#define KBE_YUV_ABI_VERSION 1\n'), ('kbe_transition.h', '#define KBE_TRANSITION_ABI_VERSION 1\n'), ('kbe_overlay.h', '#define KBE_OVERLAY_ABI_VERSION 1\n')],
    ('kbe_grade_u8', NULL_CALL, 'kbe_grade_u8: null frames_u8'),
    ('kbe_grade_u8', None, lambda frames: ((frames, 1.0, 4, 4, 12, frames, 2, frames, None), (frames, 1, 4, 4, c_size_t(12), frames, 2, frames, None),
                                           (frames, 1, 4, 4, 12, frames, 0.5, frames, None), (frames, 1, 4, 4, 12, frames, 2, frames))),
    [('kbe_grade_abi_version', 0, (1,)), ('kbe_grade_u8', 9, NULL_CALL + (0,)), ('kbe_grade_u8', 9, NULL_CALL[:-1])],
    ['kbe_overlay_u8', 'kbe_transition_u8', 'kbe_yuv420_u8', 'kbe_shutter_mean_u8', 'kbe_dof_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_grade_u8', lambda at: ((c_void_p * 2)(at, at + 1024), 2, 16, 17, 48, at + 4096, 5, (c_int32 * 2)(256, 257), None),
     'kbe_grade_u8 failed (-1): kbe_grade_u8: an element of strength outside 0..256'),
    ['kbe_grade_u8'], set())
# what the other headers' modules declare: the lists this header must leave as they are
OTHERS = {'gif': list(thb.GIF.protos), 'area': list(thb.AREA.protos), 'crop_area': ['kbe_crop_area_abi_version', 'kbe_crop_area_u8'], 'dof': ['kbe_dof_abi_version', 'kbe_dof_u8'],
          'shutter': ['kbe_shutter_abi_version', 'kbe_shutter_mean_u8'], 'yuv': ['kbe_yuv_abi_version', 'kbe_yuv420_bytes', 'kbe_yuv420_u8'],
          'transition': ['kbe_transition_abi_version', 'kbe_transition_u8'], 'overlay': ['kbe_overlay_abi_version', 'kbe_overlay_u8']}


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(GRADE)
    from ken_burns_effect_amd import grade
    assert list(grade.prototypes()) == ['kbe_grade_abi_version', 'kbe_grade_u8']


def test_the_library_exports_them_beside_the_others():
    thb.test_the_library_exports_them_with_the_headers_types(GRADE)
    from ken_burns_effect_amd import _native, grade
    lib = grade.load()
    assert lib is _native.load() and lib.kbe_grade_abi_version() == 1 == grade.ABI_VERSION
    for name, entries in OTHERS.items():
        module = importlib.import_module('ken_burns_effect_amd.' + name)
        assert module.load() is lib and getattr(lib, entries[0])() == 1


def test_the_older_headers_and_their_bindings_are_what_they_were():
    from ken_burns_effect_amd import _native, grade
    b = GRADE
    grade.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for name, entries in OTHERS.items():
        other = importlib.import_module('ken_burns_effect_amd.' + name)
        assert list(other.prototypes()) == entries and other.ABI_VERSION == 1
    # grade.py is the only module of the package whose text names the header's prefix, and it names no entry of another header
    package = os.path.dirname(grade.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and b.prefix in open(os.path.join(package, name)).read()]
    assert naming == ['grade.py']
    with open(grade.__file__) as f:
        text = f.read()
    foreign = set(_native.SYMBOLS) | {entry for entries in OTHERS.values() for entry in entries}
    assert not [entry for entry in sorted(foreign) if entry in text]
    name, args, text = b.null_call
    assert grade._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(GRADE)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(GRADE)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(GRADE)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(GRADE)


def test_the_header_states_the_cut_into_launches_and_the_makefile_builds_the_source():
    from ken_burns_effect_amd import grade
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'kbe_grade.hip')) as f:
        text = f.read()
    assert 'kFramesPerLaunch = KBE_GRADE_FRAMES_PER_LAUNCH' in text and 'asm' not in text.replace('assembl', '')
    assert grade.FRAMES_PER_LAUNCH == 12
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'Makefile')) as f:
        text = f.read()
    assert ' kbe_grade.hip' in text and ' kbe_grade_block.h' in text and '../../include/kbe_grade.h' in text
