"""The binding of include/kbe_gif.h (ken-burns-effect_amd/gif.py): the header parses to exactly its six entries, the built library exports
them beside those of kbe.h, ctypes holds every call to the header's types, and kbe.h, its binding and its ABI number are what they were.  No GPU."""
import ast
import ctypes
import os
from ctypes import c_int, c_size_t, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['kbe_gif_abi_version', 'kbe_gif_bound', 'kbe_gif_scratch_bytes', 'kbe_gif_encode', 'kbe_gif_histogram', 'kbe_gif_lut']


@pytest.fixture(scope='module')
def gif():
    from ken_burns_effect_amd import gif as module
    return module


def test_the_header_parses_to_exactly_the_six_entries(gif):
    p, i, z = c_void_p, c_int, c_size_t
    protos = gif.prototypes()
    assert list(protos) == ENTRIES
    assert protos['kbe_gif_abi_version'] == (c_int, [])
    assert protos['kbe_gif_bound'] == (c_size_t, [i, i])
    assert protos['kbe_gif_scratch_bytes'] == (c_size_t, [i, i, i])
    # the shared contract's frames, n, W, H, stride; flags, dither, delay, lut; scratch, out, cap, offsets, status, stream
    assert protos['kbe_gif_encode'] == (c_int, [p, i, i, i, i, i, i, i, p, p, p, z, p, p, p])
    assert protos['kbe_gif_histogram'] == (c_int, [p, i, i, i, i, i, p, p])
    assert protos['kbe_gif_lut'] == (c_int, [p, i, p, p])
    with open(gif.HEADER_PATH) as f:
        text = f.read()
    assert '#define KBE_GIF_ABI_VERSION 1\n' in text and '#define KBE_GIF_BGR 1\n' in text and gif.KBE_GIF_BGR == 1 and gif.ABI_VERSION == 1


def test_the_library_exports_them_with_the_headers_types(gif):
    lib = gif.load()
    assert lib.kbe_gif_abi_version() == 1
    for name, (restype, argtypes) in gif.prototypes().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_kbe_h_and_its_binding_are_what_they_were(gif):
    from ken_burns_effect_amd import _native
    gif.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith('kbe_gif') for name in _native.SYMBOLS)
    with open(_native.__file__) as f:
        assert 'kbe_gif' not in f.read()
    with open(os.path.join(ROOT, 'include', 'kbe.h')) as f:
        text = f.read()
    assert 'kbe_gif' not in text and 'KBE_GIF' not in text and '#define KBE_ABI_VERSION 13\n' in text
    # the two handles are one library: the typed entries of kbe.h carry no GIF types, and an error text set through one is read through the other
    assert _native.load().kbe_abi_version() == 13
    assert gif._raw('kbe_gif_lut', None, 0, None, None) == -1 and _native.load().kbe_last_error().decode() == 'kbe_gif_lut: null palette or lut'


def test_ctypes_refuses_a_wrong_call_before_it_is_made(gif):
    lib = gif.load()
    assert lib.kbe_gif_bound(1, 1) == 25 == lib.kbe_gif_bound(c_int(1), 1)
    for wrong in ((16.0, 17), (c_size_t(16), 17), (16,)):
        with pytest.raises((ctypes.ArgumentError, TypeError)):
            lib.kbe_gif_bound(*wrong)


def test_a_surplus_or_missing_argument_is_refused(gif):
    from ken_burns_effect_amd import _native
    for args in ((16, 17, 18), (16,)):          # (ctypes alone accepts the first: cdecl)
        with pytest.raises(_native.KbeError, match='kbe_gif_bound takes 2 arguments, got %d' % len(args)):
            gif._raw('kbe_gif_bound', *args)
    with pytest.raises(_native.KbeError, match='kbe_gif_no_such_entry'):
        gif._call('kbe_gif_no_such_entry')
    with pytest.raises(_native.KbeError, match='kbe_png_bound is not an entry of include/kbe_gif.h'):
        gif._raw('kbe_png_bound', 4, 4)


def test_call_reports_a_refusal_with_the_librarys_text(gif):
    from ken_burns_effect_amd import _native
    memory = (ctypes.c_uint64 * 1024)()                                     # host memory: the entry refuses before anything reads or writes it
    at = ctypes.addressof(memory)
    frames = (c_void_p * 3)(at + 4096, at + 4096, at + 4096)
    with pytest.raises(_native.KbeError) as e:
        gif._call('kbe_gif_encode', frames, 3, 16, 17, 48, 0, 0, 70000, at + 512, at, at + 1024, 1024, at + 2048, at + 3072, None)
    assert str(e.value) == 'kbe_gif_encode failed (-1): kbe_gif_encode: delay_cs outside 0..65535'
    assert not any(memory)


def test_every_call_site_passes_the_headers_number_of_arguments(gif):
    """An ast walk of gif.py: every _call(...) and _raw(...) names an entry of the header by a string literal and passes its argument count."""
    with open(gif.__file__) as f:
        tree = ast.parse(f.read())
    protos = gif.prototypes()
    sites = [(node.args[0], node.args[1:]) for fn in tree.body if isinstance(fn, ast.FunctionDef) and fn.name not in ('_call', '_raw') for node in ast.walk(fn)
             if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ('_call', '_raw')]
    assert len(sites) >= 3
    for name, args in sites:
        assert isinstance(name, ast.Constant) and name.value in protos and not any(isinstance(a, ast.Starred) for a in args), ast.dump(name)
        assert len(args) == len(protos[name.value][1]), '%s takes %d arguments, gif.py passes %d' % (name.value, len(protos[name.value][1]), len(args))
    assert {name.value for name, _ in sites} == {'kbe_gif_encode', 'kbe_gif_histogram', 'kbe_gif_lut'}
    # what gif.py takes from the library itself: the entries that return a size or a number
    direct = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith('kbe_')}
    assert direct == {'kbe_gif_abi_version', 'kbe_gif_scratch_bytes', 'kbe_last_error'}
