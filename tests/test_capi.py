"""The C-ABI library loads without a GPU and exports every symbol include/kbe.h declares."""
import ctypes
import os
import re

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, 'include', 'kbe.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(kbe_[a-z0-9_]+)\s*\(', text)))


def test_header_and_binding_agree():
    """The names the binding's parser (_cabi.prototypes, through _native.prototypes) reads from the header are the ones this file's own
    regular expression finds."""
    from ken_burns_effect_amd import _native
    assert _declared() == sorted(_native.prototypes()) == sorted(_native.SYMBOLS)


def test_library_exports_every_declared_symbol():
    from ken_burns_effect_amd import _native
    assert os.path.exists(_native.LIB_PATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    lib.kbe_abi_version.restype = ctypes.c_int
    assert lib.kbe_abi_version() == _native.ABI_VERSION
    assert _native.load() is not None


def test_library_is_a_gfx950_code_object():
    from ken_burns_effect_amd import _native
    import re
    blob = open(_native.LIB_PATH, 'rb').read()
    # the offload bundle holds exactly one device code object, for gfx950: single target, no dual paths.  (The host side of
    # rocprim's radix sort carries a table of architecture NAMES for its tuning dispatch; names are not code objects.)
    targets = set(re.findall(rb'amdgcn-amd-amdhsa--(gfx[0-9a-f]+)', blob))
    assert targets == {b'gfx950'}, targets
    assert b'nvptx' not in blob and b'sm_80' not in blob and b'sm_90' not in blob


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, 'ken-burns-effect_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(dirpath, f)).read()
                assert 'kbe_oracle' not in src.replace('oracle/kbe_oracle.c', '').replace('oracle/kbe_oracle', ''), f
                assert 'import oracle' not in src and 'from oracle' not in src, f


def _header_flags():
    """({name: value}, {name: body in `n`}) of the `#define KBE_VIDEO_*` / `#define KBE_STAGE_*` lines of include/kbe.h."""
    text = open(os.path.join(ROOT, 'include', 'kbe.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    plain = {name: int(value) for name, value in re.findall(r'^#define (KBE_(?:VIDEO|STAGE)_[A-Z_]+)[ \t]+(\d+)[ \t]*$', text, flags=re.M)}
    macros = dict(re.findall(r'^#define (KBE_(?:VIDEO|STAGE)_[A-Z_]+)\(n\)[ \t]+(.+?)[ \t]*$', text, flags=re.M))
    return plain, macros


def test_flag_constants_of_the_binding_are_the_headers():
    """Every KBE_VIDEO_* / KBE_STAGE_* name the binding (and the module that decides a call's shape) defines has the header's
    value -- the function-like macros for every n they take: 1..4 frames per launch either route, 1..12 on the fused one."""
    from ken_burns_effect_amd import _native, video_shape
    plain, macros = _header_flags()
    assert len(plain) >= 20 and set(macros) == {'KBE_VIDEO_FILL_GROUP', 'KBE_VIDEO_GROUP'}
    seen = set()
    for mod in (_native, video_shape):
        for name, value in vars(mod).items():
            if not name.startswith(('KBE_VIDEO_', 'KBE_STAGE_')):
                continue
            seen.add(name)
            if name in macros:
                for n in range(1, 5 if name == 'KBE_VIDEO_FILL_GROUP' else 13):
                    assert value(n) == eval(macros[name], {'n': n}), (name, n)
            else:
                assert name in plain and value == plain[name], name
    # the flags of kbe_render_video, all of them, and the build bits of the one-frame and group entries
    assert seen >= {n for n in plain if n.startswith('KBE_VIDEO_')} | set(macros) | {'KBE_STAGE_FUSED_LEAN', 'KBE_STAGE_FUSED_ROOMY'}
    assert video_shape.launch_flags(True, 4) == 1 | (3 << 1) and video_shape.launch_flags(False, 12) == 11 << 5
