"""The bindings of include/kbe_gif.h (ken-burns-effect_amd/gif.py) and include/kbe_area.h (area.py), one table for the two: a header parses to
exactly its entries, the built library exports them beside those of kbe.h, ctypes holds every call to the header's types, every module refuses
the others' entries, and the older headers, their bindings and their ABI numbers are what they were.  All three modules call through ONE handle
of the library, the one _native.load() opened last.  No GPU."""
import ast
import collections
import ctypes
import importlib
import os
import shutil
from ctypes import c_int, c_size_t, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p, i, z = c_void_p, c_int, c_size_t
NULL_REDUCE = (None, 1, 4, 4, 12, None, 2, 2, 6, None)

# module: of the package; prefix: of the entries' names; protos: what the header parses to, in its order; abi: the entry that returns the ABI
# number; defines, absent: what the header's text holds and does not; constants: the module's values of them; older: the headers that were
# there before this one, each with its ABI line; null_call: a call the entry refuses by its return code, with the library's text; typed:
# (an entry, a good call of it and its value or None, calls ctypes itself refuses); miscounted: (entry, the header's count, arguments);
# foreign: entries of the other headers; refused: (entry, its arguments by the address of 8 KiB of host memory, the message of _call);
# sites, direct: the entries gif.py / area.py calls through _call and _raw, and what it takes from the library itself
Binding = collections.namedtuple('Binding', 'module prefix protos abi defines absent constants older null_call typed miscounted foreign refused sites direct')
GIF = Binding(
    'gif', 'kbe_gif',
    {'kbe_gif_abi_version': (c_int, []), 'kbe_gif_bound': (c_size_t, [i, i]), 'kbe_gif_scratch_bytes': (c_size_t, [i, i, i]),
     # the shared contract's frames, n, W, H, stride; flags, dither, delay, lut; scratch, out, cap, offsets, status, stream
     'kbe_gif_encode': (c_int, [p, i, i, i, i, i, i, i, p, p, p, z, p, p, p]), 'kbe_gif_histogram': (c_int, [p, i, i, i, i, i, p, p]), 'kbe_gif_lut': (c_int, [p, i, p, p])},
    'kbe_gif_abi_version', ['#define KBE_GIF_ABI_VERSION 1\n', '#define KBE_GIF_BGR 1\n'], [], {'KBE_GIF_BGR': 1, 'ABI_VERSION': 1},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n')],
    ('kbe_gif_lut', (None, 0, None, None), 'kbe_gif_lut: null palette or lut'),
    ('kbe_gif_bound', ((1, 1), 25), lambda frames: ((16.0, 17), (c_size_t(16), 17), (16,))),
    [('kbe_gif_bound', 2, (16, 17, 18)), ('kbe_gif_bound', 2, (16,))],          # (ctypes alone accepts a surplus argument: cdecl)
    ['kbe_png_bound', 'kbe_area_abi_version'],
    ('kbe_gif_encode', lambda at: ((c_void_p * 3)(at + 4096, at + 4096, at + 4096), 3, 16, 17, 48, 0, 0, 70000, at + 512, at, at + 1024, 1024, at + 2048, at + 3072, None),
     'kbe_gif_encode failed (-1): kbe_gif_encode: delay_cs outside 0..65535'),
    ['kbe_gif_encode', 'kbe_gif_histogram', 'kbe_gif_lut'], {'kbe_gif_scratch_bytes'})
AREA = Binding(
    'area', 'kbe_area',
    # frames, n, W, H, stride; out, w, h, out stride; stream
    {'kbe_area_abi_version': (c_int, []), 'kbe_area_reduce_u8': (c_int, [p, i, i, i, i, p, i, i, i, p])},
    'kbe_area_abi_version', ['#define KBE_AREA_ABI_VERSION 1\n'], ['KBE_AREA_BGR'], {'ABI_VERSION': 1},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n')],
    ('kbe_area_reduce_u8', NULL_REDUCE, 'kbe_area_reduce_u8: null frames_u8'),
    ('kbe_area_reduce_u8', None, lambda frames: ((frames, 1.0, 4, 4, 12, frames, 2, 2, 6, None), (frames, 1, 4, 4, 12, frames, 2, 2, c_size_t(6), None), (frames, 1, 4, 4, 12, frames, 2, 2, 6))),
    [('kbe_area_abi_version', 0, (1,)), ('kbe_area_reduce_u8', 10, NULL_REDUCE + (0,)), ('kbe_area_reduce_u8', 10, NULL_REDUCE[:-1])],
    ['kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_area_reduce_u8', lambda at: ((c_void_p * 2)(at, at + 1024), 2, 16, 17, 48, (c_void_p * 2)(at + 4096, at + 6144), 17, 4, 51, None),
     'kbe_area_reduce_u8 failed (-1): kbe_area_reduce_u8: w outside 1..W: the entry only reduces'),
    ['kbe_area_reduce_u8'], set())
BINDINGS = [GIF, AREA]         # in the order the headers came: a header's `older` bindings are the ones in front of it
each_binding = pytest.mark.parametrize('b', BINDINGS, ids=lambda b: b.module)


def module_of(b):
    return importlib.import_module('ken_burns_effect_amd.' + b.module)


def assert_typed(lib, protos):
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


@each_binding
def test_the_header_parses_to_exactly_its_entries(b):
    module = module_of(b)
    protos = module.prototypes()
    assert list(protos) == list(b.protos)
    for name, proto in b.protos.items():
        assert protos[name] == proto, name
    with open(module.HEADER_PATH) as f:
        text = f.read()
    assert all(line in text for line in b.defines) and not any(word in text for word in b.absent)
    assert all(getattr(module, name) == value for name, value in b.constants.items())


@each_binding
def test_the_library_exports_them_with_the_headers_types(b):
    module = module_of(b)
    lib = module.load()
    assert getattr(lib, b.abi)() == 1
    assert_typed(lib, module.prototypes())


@each_binding
def test_the_older_headers_and_their_bindings_are_what_they_were(b):
    from ken_burns_effect_amd import _native
    module = module_of(b)
    module.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    with open(_native.__file__) as f:
        assert b.prefix not in f.read()
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for older in BINDINGS[:BINDINGS.index(b)]:
        # (gif.py reaches the reduction through area.reduce alone: it names no entry of kbe_area.h)
        other = module_of(older)
        assert list(other.prototypes()) == list(older.protos) and not any(name.startswith(b.prefix) for name in other.prototypes())
        assert getattr(other.load(), older.abi)() == 1
        with open(other.__file__) as f:
            assert b.prefix not in f.read()
    # one library: the typed entries of kbe.h carry none of this header's types, and an error text set through this module is read through kbe.h's
    name, args, text = b.null_call
    assert module._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


@each_binding
def test_ctypes_refuses_a_wrong_call_before_it_is_made(b):
    lib = module_of(b).load()
    name, good, wrong = b.typed
    fn = getattr(lib, name)
    if good is not None:
        assert fn(*good[0]) == good[1] == fn(c_int(good[0][0]), *good[0][1:])
    memory = (ctypes.c_uint64 * 64)()
    for args in wrong((c_void_p * 1)(ctypes.addressof(memory))):
        with pytest.raises((ctypes.ArgumentError, TypeError)):
            fn(*args)
    assert not any(memory)


@each_binding
def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(b):
    from ken_burns_effect_amd import _native
    module = module_of(b)
    for name, count, args in b.miscounted:
        with pytest.raises(_native.KbeError, match='%s takes %d arguments, got %d' % (name, count, len(args))):
            module._raw(name, *args)
    with pytest.raises(_native.KbeError, match=b.prefix + '_no_such_entry'):
        module._call(b.prefix + '_no_such_entry')
    for name in b.foreign:
        with pytest.raises(_native.KbeError, match='%s is not an entry of include/%s.h' % (name, b.prefix)):
            module._raw(name, 4, 4)


@each_binding
def test_call_reports_a_refusal_with_the_librarys_text(b):
    from ken_burns_effect_amd import _native
    memory = (ctypes.c_uint64 * 1024)()                                     # host memory: the entry refuses before anything reads or writes it
    name, args, text = b.refused
    with pytest.raises(_native.KbeError) as e:
        module_of(b)._call(name, *args(ctypes.addressof(memory)))
    assert str(e.value) == text
    assert not any(memory)


@each_binding
def test_every_call_site_passes_the_headers_number_of_arguments(b):
    """An ast walk of the module: every _call(...) and _raw(...) names an entry of the header by a string literal and passes its argument count."""
    module = module_of(b)
    with open(module.__file__) as f:
        tree = ast.parse(f.read())
    protos = module.prototypes()
    sites = [(node.args[0], node.args[1:]) for fn in tree.body if isinstance(fn, ast.FunctionDef) and fn.name not in ('_call', '_raw') for node in ast.walk(fn)
             if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ('_call', '_raw')]
    for name, args in sites:
        assert isinstance(name, ast.Constant) and name.value in protos and not any(isinstance(a, ast.Starred) for a in args), ast.dump(name)
        assert len(args) == len(protos[name.value][1]), '%s takes %d arguments, %s.py passes %d' % (name.value, len(protos[name.value][1]), b.module, len(args))
    assert sorted(name.value for name, _ in sites) == b.sites               # one site per entry
    # what the module takes from the library itself: the entries that return a size (the ABI number and the error text are _cabi.Header's)
    assert {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith('kbe_')} == b.direct


def test_after_a_tools_switch_of_libraries_every_module_calls_the_new_one(monkeypatch, tmp_path):
    """tools/*.py switch to a variant build with `_native._lib, _native._kernels, _native.LIB_PATH = None, None, path`: gif.py and area.py then
    call that library too, through the same handle, typed from all three headers."""
    from ken_burns_effect_amd import _native, area, gif
    before = _native.load()
    assert gif.load() is area.load() is before
    variant = str(tmp_path / 'libkbe_variant.so')
    shutil.copy(_native.LIB_PATH, variant)
    for name, value in (('_lib', None), ('_kernels', None), ('LIB_PATH', variant)):
        monkeypatch.setattr(_native, name, value)
    lib = _native.load()
    assert gif.load() is area.load() is lib and lib is not before and lib._name == variant
    for module in (_native, gif, area):
        assert_typed(lib, module.prototypes())
    assert lib.kbe_gif_bound(1, 1) == 25 and lib.kbe_abi_version() == 13 and lib.kbe_gif_abi_version() == 1 == lib.kbe_area_abi_version()
    K = _native.kernels()
    assert K.lib is lib and K._raw('kbe_mjpeg_bound', 16, 17) == 5627
    for name in ('kbe_gif_bound', 'kbe_area_abi_version'):                  # not entries of kbe.h, whatever the handle exports and types
        with pytest.raises(_native.KbeError, match='%s is not an entry of include/kbe.h' % name):
            K._raw(name, 1, 1)
    assert gif._raw('kbe_gif_lut', None, 0, None, None) == -1 and lib.kbe_last_error().decode() == 'kbe_gif_lut: null palette or lut'
    assert area._raw('kbe_area_reduce_u8', *NULL_REDUCE) == -1 and lib.kbe_last_error().decode() == 'kbe_area_reduce_u8: null frames_u8'
