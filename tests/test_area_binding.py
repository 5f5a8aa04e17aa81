"""The binding of include/kbe_area.h (ken-burns-effect_amd/area.py): the header parses to exactly its two entries, the built library exports
them beside those of kbe.h and kbe_gif.h, ctypes holds every call to the header's types, and kbe.h, kbe_gif.h, their bindings and their ABI
numbers are what they were.  No GPU."""
import ast
import ctypes
import os
from ctypes import c_int, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['kbe_area_abi_version', 'kbe_area_reduce_u8']


@pytest.fixture(scope='module')
def area():
    from ken_burns_effect_amd import area as module
    return module


def test_the_header_parses_to_exactly_the_two_entries(area):
    p, i = c_void_p, c_int
    protos = area.prototypes()
    assert list(protos) == ENTRIES
    assert protos['kbe_area_abi_version'] == (c_int, [])
    # frames, n, W, H, stride; out, w, h, out stride; stream
    assert protos['kbe_area_reduce_u8'] == (c_int, [p, i, i, i, i, p, i, i, i, p])
    with open(area.HEADER_PATH) as f:
        text = f.read()
    assert '#define KBE_AREA_ABI_VERSION 1\n' in text and area.ABI_VERSION == 1 and 'KBE_AREA_BGR' not in text


def test_the_library_exports_them_with_the_headers_types(area):
    lib = area.load()
    assert lib.kbe_area_abi_version() == 1
    for name, (restype, argtypes) in area.prototypes().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_kbe_h_kbe_gif_h_and_their_bindings_are_what_they_were(area):
    from ken_burns_effect_amd import _native, gif
    area.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith('kbe_area') for name in _native.SYMBOLS)
    with open(_native.__file__) as f:
        assert 'kbe_area' not in f.read()
    for header, number in (('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n')):
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert 'kbe_area' not in text and 'KBE_AREA' not in text and number in text
    assert len(gif.prototypes()) == 6 and not any(name.startswith('kbe_area') for name in gif.prototypes())
    assert _native.load().kbe_abi_version() == 13 and gif.load().kbe_gif_abi_version() == 1
    # gif.py reaches the reduction through area.reduce alone: it names no entry of kbe_area.h
    with open(gif.__file__) as f:
        assert 'kbe_area' not in f.read()
    # the handles are one library: an error text set through this one is read through kbe.h's
    assert area._raw('kbe_area_reduce_u8', None, 1, 4, 4, 12, None, 2, 2, 6, None) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_area_reduce_u8: null frames_u8'


def test_ctypes_refuses_a_wrong_call_before_it_is_made(area):
    lib = area.load()
    memory = (ctypes.c_uint64 * 64)()
    frames = (c_void_p * 1)(ctypes.addressof(memory))
    for wrong in ((frames, 1.0, 4, 4, 12, frames, 2, 2, 6, None), (frames, 1, 4, 4, 12, frames, 2, 2, ctypes.c_size_t(6), None), (frames, 1, 4, 4, 12, frames, 2, 2, 6)):
        with pytest.raises((ctypes.ArgumentError, TypeError)):
            lib.kbe_area_reduce_u8(*wrong)
    assert not any(memory)


def test_a_surplus_or_missing_argument_is_refused(area):
    from ken_burns_effect_amd import _native
    for args in ((1,), (None, 1, 4, 4, 12, None, 2, 2, 6, None, 0), (None, 1, 4, 4, 12, None, 2, 2, 6)):          # (ctypes alone accepts a surplus one: cdecl)
        name = 'kbe_area_abi_version' if len(args) == 1 else 'kbe_area_reduce_u8'
        with pytest.raises(_native.KbeError, match='%s takes %d arguments, got %d' % (name, 0 if len(args) == 1 else 10, len(args))):
            area._raw(name, *args)
    with pytest.raises(_native.KbeError, match='kbe_area_no_such_entry'):
        area._call('kbe_area_no_such_entry')
    with pytest.raises(_native.KbeError, match='kbe_gif_bound is not an entry of include/kbe_area.h'):
        area._raw('kbe_gif_bound', 4, 4)


def test_call_reports_a_refusal_with_the_librarys_text(area):
    from ken_burns_effect_amd import _native
    memory = (ctypes.c_uint64 * 1024)()                                     # host memory: the entry refuses before anything reads or writes it
    at = ctypes.addressof(memory)
    frames, out = (c_void_p * 2)(at, at + 1024), (c_void_p * 2)(at + 4096, at + 6144)
    with pytest.raises(_native.KbeError) as e:
        area._call('kbe_area_reduce_u8', frames, 2, 16, 17, 48, out, 17, 4, 51, None)
    assert str(e.value) == 'kbe_area_reduce_u8 failed (-1): kbe_area_reduce_u8: w outside 1..W: the entry only reduces'
    assert not any(memory)


def test_every_call_site_passes_the_headers_number_of_arguments(area):
    """An ast walk of area.py: every _call(...) and _raw(...) names an entry of the header by a string literal and passes its argument count."""
    with open(area.__file__) as f:
        tree = ast.parse(f.read())
    protos = area.prototypes()
    sites = [(node.args[0], node.args[1:]) for fn in tree.body if isinstance(fn, ast.FunctionDef) and fn.name not in ('_call', '_raw') for node in ast.walk(fn)
             if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ('_call', '_raw')]
    assert len(sites) >= 1
    for name, args in sites:
        assert isinstance(name, ast.Constant) and name.value in protos and not any(isinstance(a, ast.Starred) for a in args), ast.dump(name)
        assert len(args) == len(protos[name.value][1]), '%s takes %d arguments, area.py passes %d' % (name.value, len(protos[name.value][1]), len(args))
    assert {name.value for name, _ in sites} == {'kbe_area_reduce_u8'}
    direct = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith('kbe_')}
    assert direct == {'kbe_area_abi_version', 'kbe_last_error'}
