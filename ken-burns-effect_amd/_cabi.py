"""The prototypes of a C ABI header (include/kbe.h, include/kbe_jpeg.h) as ctypes types: the header is the contract, and ctypes holds every
call to it -- a float for an int, a value of another width or a missing argument is refused before the call.  Not a C parser: it knows the
few types these headers use and raises on any other."""
import ctypes
import re

_BY_VALUE = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'double': ctypes.c_double, 'float': ctypes.c_float, 'kbe_stream_t': ctypes.c_void_p}


def _ctype(decl, name, returned=False):
    """The ctypes type of a parameter `decl` ("const float* shift3", "int W") or of a return type of the entry `name`."""
    words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
    if '*' in words:
        if not returned:
            return ctypes.c_void_p
        kind = ctypes.c_char_p if words == ['char', '*'] else None
    else:
        kind = _BY_VALUE.get(' '.join(words if returned or len(words) == 1 else words[:-1]))       # (a parameter's last word is its name)
    if kind is None or (returned and kind is ctypes.c_void_p):
        raise ValueError('%s: no ctypes type for %r' % (name, decl.strip()))
    return kind


def prototypes(text, api):
    """{name: (restype, [argtypes])}, in declaration order, of the declarations `api` marks (KBE_API, KBE_JPEG_API) in a header's text."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    protos = {}
    for returned, name, params in re.findall(r'\b%s\s+([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*;' % re.escape(api), text):
        params = [] if params.strip() == 'void' else params.split(',')
        protos[name] = (_ctype(returned, name, returned=True), [_ctype(p, name) for p in params])
    return protos


def bind(lib, protos):
    """Sets the prototypes on the functions of a ctypes library (which must export every one of them)."""
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib
