"""The binding is typed from the headers: _cabi parses include/kbe.h and include/kbe_jpeg.h, _native.load() sets what it finds on every
entry, and HipKernels._call holds every wrapper to the header's argument count -- so a wrapper with a wrong, missing or surplus argument
fails here, without a GPU, and not as corrupt device memory."""
import ast
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_size_t, c_void_p

import pytest

import test_capi
from conftest import ROOT

CRAFTED = """
/* a block comment with a prototype in it:
   MY_API int commented_out(int a); */
// MY_API int behind_slashes(int a);
typedef void* kbe_stream_t;
#define MY_API __attribute__((visibility("default")))
MY_API int no_arguments(void);
MY_API const char* text(void);   // MY_API int trailing(int a);
MY_API size_t size(int W, double focal, float threshold, size_t n);
MY_API int spread(const uint8_t* const* frames,
                  void* const* sets,   /* MY_API int inside(int a); */
                  const kbe_stream_t* lanes, kbe_stream_t stream);
int not_exported(int a);
"""
SIZES = {'kbe_frame_scratch_bytes', 'kbe_video_scratch_stride', 'kbe_video_stage_bytes', 'kbe_cloud_pack_bytes', 'kbe_mjpeg_bound', 'kbe_mjpeg_scratch_bytes',
         'kbe_png_bound', 'kbe_png_scratch_bytes'}
STARRED = {'encode_raw'}         # the wrappers whose _call spreads a sequence: their counts are checked by the call itself


def _header(name, api):
    from ken_burns_effect_amd import _cabi
    with open(os.path.join(ROOT, 'include', name)) as f:
        return _cabi.prototypes(f.read(), api)


@pytest.fixture(scope='module')
def kbe():
    return _header('kbe.h', 'KBE_API')


# -- the parser ---------------------------------------------------------------------------
def test_the_parser_on_a_crafted_header():
    from ken_burns_effect_amd import _cabi
    protos = _cabi.prototypes(CRAFTED, 'MY_API')
    assert list(protos) == ['no_arguments', 'text', 'size', 'spread']          # declaration order; nothing from a comment, nothing unmarked
    assert protos['no_arguments'] == (c_int, [])
    assert protos['text'] == (c_char_p, [])
    assert protos['size'] == (c_size_t, [c_int, c_double, c_float, c_size_t])
    assert protos['spread'] == (c_int, [c_void_p, c_void_p, c_void_p, c_void_p])


@pytest.mark.parametrize('decl', ['MY_API int f(long x);', 'MY_API int f(int a, unsigned b);', 'MY_API long f(int a);', 'MY_API void* f(int a);', 'MY_API int f();'])
def test_the_parser_refuses_a_type_it_does_not_know(decl):
    from ken_burns_effect_amd import _cabi
    with pytest.raises(ValueError, match=r'\bf: no ctypes type for'):
        _cabi.prototypes(decl, 'MY_API')


def test_the_real_headers_names_are_the_ones_test_capi_finds(kbe):
    jpeg = _header('kbe_jpeg.h', 'KBE_JPEG_API')
    assert sorted(kbe) == test_capi._declared() and len(kbe) == 48
    assert list(jpeg) == ['kbe_jpeg_bound', 'kbe_jpeg_encode', 'kbe_jpeg_encode_batch']
    assert jpeg['kbe_jpeg_bound'] == (c_size_t, [c_int, c_int])
    assert jpeg['kbe_jpeg_encode'] == (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p])
    assert jpeg['kbe_jpeg_encode_batch'] == (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int])


def test_the_real_headers_return_types(kbe):
    assert {name for name, (restype, _) in kbe.items() if restype is c_size_t} == SIZES
    assert kbe['kbe_last_error'] == (c_char_p, [])
    assert {name for name, (restype, _) in kbe.items() if restype is not c_int} == SIZES | {'kbe_last_error'}


def test_the_real_headers_parameter_lists(kbe):
    p, i, d, z, f = c_void_p, c_int, c_double, c_size_t, c_float
    assert kbe['kbe_render_video'][1] == [p, p, p, i, i, i, d, i, p, p, i, i, p, p, i, p, i, i, p, d, i, p, p, i, p, d] and len(kbe['kbe_render_video'][1]) == 26
    assert kbe['kbe_png_encode'][1] == [p, i, i, i, i, i, p, p, z, p, p, p]
    assert kbe['kbe_mjpeg_encode'][1] == [p, i, i, i, i, i, i, p, p, z, p, p, p]
    assert kbe['kbe_frame_scratch_init_sets'][1] == [p, z, i, i, i, p]
    assert kbe['kbe_laplacian_valid'][1] == [p, p, i, i, i, f, p, p]
    assert kbe['kbe_device_info'][1] == [i, p, i] and kbe['kbe_abi_version'][1] == []


# -- the loaded library -------------------------------------------------------------------
def test_every_entry_of_the_loaded_library_carries_the_headers_types(kbe):
    from ken_burns_effect_amd import _native
    lib = _native.load()
    assert tuple(_native.SYMBOLS) == tuple(kbe) == tuple(_native.prototypes())
    for name, (restype, argtypes) in kbe.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    from ken_burns_effect_amd import _native
    lib = _native.load()
    assert lib.kbe_mjpeg_bound(16, 17) == 5627 == lib.kbe_mjpeg_bound(c_int(16), 17)
    for wrong in ((16.0, 17), (c_size_t(16), 17), (16,)):
        with pytest.raises((ctypes.ArgumentError, TypeError)):
            lib.kbe_mjpeg_bound(*wrong)


def test_call_refuses_an_argument_count_that_is_not_the_headers():
    from ken_burns_effect_amd import _native
    K = _native.HipKernels()
    for args in ((16, 17, 18), (16,)):          # (ctypes alone accepts the first: cdecl)
        with pytest.raises(_native.KbeError, match='kbe_mjpeg_bound takes 2 arguments, got %d' % len(args)):
            K._call('kbe_mjpeg_bound', *args)
    with pytest.raises(_native.KbeError, match='kbe_no_such_entry'):
        K._call('kbe_no_such_entry')


def test_call_reports_a_refusal_with_the_librarys_text():
    from ken_burns_effect_amd import _native
    K = _native.HipKernels()
    memory = (ctypes.c_uint64 * 1024)()                                     # host memory: the entry refuses before anything reads or writes it
    at = ctypes.addressof(memory)
    frames = (c_void_p * 3)(at + 4096, at + 4096, at + 4096)
    args = (frames, 0, 16, 17, 48, 92, 0, at, at + 1024, 1024, at + 2048, at + 3072, None)
    with pytest.raises(_native.KbeError) as e:
        K._call('kbe_mjpeg_encode', *args)
    assert str(e.value) == 'kbe_mjpeg_encode failed (-1): kbe_mjpeg_encode: bad frames or size'
    with pytest.raises(_native.KbeError) as e:
        K._call('kbe_mjpeg_encode', *args, what='the label')
    assert str(e.value) == 'the label failed (-1): kbe_mjpeg_encode: bad frames or size'


def test_load_names_a_missing_header(monkeypatch, tmp_path):
    from ken_burns_effect_amd import _native
    missing = str(tmp_path / 'include' / 'kbe.h')
    monkeypatch.setattr(_native.HEADER, 'path', missing)
    monkeypatch.setattr(_native.HEADER, '_protos', None)
    monkeypatch.setattr(_native.HEADER, '_bound', None)
    monkeypatch.setattr(_native, '_lib', None)
    with pytest.raises(_native.KbeError, match=missing):
        _native.load()


# -- the wrappers' call sites, which only a GPU executes ------------------------------------
def _call_sites():
    """(method of HipKernels, entry name node, positional arguments) of every self._call(...) and self._raw(...) in _native.py."""
    from ken_burns_effect_amd import _native
    with open(_native.__file__) as f:
        tree = ast.parse(f.read())
    methods = [fn for cls in tree.body if isinstance(cls, ast.ClassDef) and cls.name == 'HipKernels' for fn in cls.body if isinstance(fn, ast.FunctionDef)]
    return [(fn.name, node.args[0], node.args[1:]) for fn in methods if fn.name != '_call' for node in ast.walk(fn)
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ('_call', '_raw')]


def test_every_wrapper_passes_the_headers_number_of_arguments(kbe):
    sites = _call_sites()
    assert len(sites) >= 35
    starred = set()
    for where, name, args in sites:
        if any(isinstance(a, ast.Starred) for a in args):
            starred.add(where)
            continue
        assert isinstance(name, ast.Constant) and name.value in kbe, (where, ast.dump(name))
        assert len(args) == len(kbe[name.value][1]), '%s: %s takes %d arguments, the wrapper passes %d' % (where, name.value, len(kbe[name.value][1]), len(args))
    assert starred == STARRED


def test_only_entries_without_a_status_are_called_past_call():
    """What HipKernels takes from self.lib itself: the entries that return a size or a yes / no, the error text, and the function
    prepared_group_ahead binds once for its timing loops.  Every other entry goes through _call / _raw."""
    from ken_burns_effect_amd import _native
    with open(_native.__file__) as f:
        tree = ast.parse(f.read())
    cls = [c for c in tree.body if isinstance(c, ast.ClassDef) and c.name == 'HipKernels'][0]
    direct = {(fn.name, n.attr) for fn in cls.body if isinstance(fn, ast.FunctionDef) for n in ast.walk(fn)
              if isinstance(n, ast.Attribute) and n.attr.startswith('kbe_')}
    assert {name for _, name in direct} - {'kbe_last_error', 'kbe_render_frame_group_ahead'} <= SIZES
    assert {where for where, name in direct if name == 'kbe_render_frame_group_ahead'} == {'prepared_group_ahead'}


def test_every_entry_the_binding_names_is_in_the_header(kbe):
    """Every 'kbe_...' string literal and every attribute taken from a `.lib` in _native.py names an entry of include/kbe.h."""
    from ken_burns_effect_amd import _native
    with open(_native.__file__) as f:
        tree = ast.parse(f.read())
    named = {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value.startswith('kbe_') and n.value.isidentifier()}
    named |= {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith('kbe_')}
    assert len(named) >= 40 and named <= set(kbe), named - set(kbe)


# -- on the GPU: the one entry no other test reaches ----------------------------------------
@pytest.mark.gpu
def test_device_info_through_the_typed_binding():
    from ken_burns_effect_amd import _native
    lib = _native.load()
    name = ctypes.create_string_buffer(b'\xaa' * 64, 64)
    assert lib.kbe_device_info(0, name, 64) > 0 and name.value.startswith(b'gfx950')
    short = ctypes.create_string_buffer(b'\xaa' * 16, 16)
    assert lib.kbe_device_info(0, short, 4) > 0
    assert short.raw == b'gfx\0' + b'\xaa' * 12
