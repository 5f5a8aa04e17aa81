"""The prototypes of a C ABI header (include/kbe.h, kbe_gif.h, kbe_area.h, kbe_jpeg.h) as ctypes types: the header is the contract, and ctypes
holds every call to it -- a float for an int, a value of another width or a missing argument is refused before the call.  Not a C parser: it
knows the few types these headers use and raises on any other.  Header is what a module keeps of its header: the prototypes read once, an
open library typed and checked against them, and the two ways every entry is called."""
import ctypes
import os
import re

_BY_VALUE = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'double': ctypes.c_double, 'float': ctypes.c_float, 'uint32_t': ctypes.c_uint32, 'kbe_stream_t': ctypes.c_void_p}


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


class KbeError(RuntimeError):
    pass


class Header:
    """One header of the C ABI: `path`, the macro `api` that marks its entries, what messages call it (`name`: include/kbe_gif.h) and the
    library that exports them; `abi`: (the entry that returns its ABI number, the number expected, the label of the two in messages:
    '', 'GIF ', 'area ').  Opens nothing: bind, raw and call take an open ctypes.CDLL."""

    def __init__(self, path, api, name, abi=None, library='libkbe_hip.so'):
        self.path, self.api, self.name, self.abi, self.library = path, api, name, abi, library
        self._protos = None
        self._bound = None         # the handle bind saw last

    def prototypes(self):
        """{entry: (restype, [argtypes])} of every entry the header declares, in its order, read once."""
        if self._protos is None:
            if not os.path.exists(self.path):
                entries = 'the %sentries' % self.abi[2] if self.abi and self.abi[2] else 'every entry'
                raise KbeError('%s is missing: the binding takes the types of %s of %s from it' % (self.path, entries, self.library))
            with open(self.path) as f:
                self._protos = prototypes(f.read(), self.api)
        return self._protos

    def bind(self, lib):
        """`lib` with every entry of the header exported, typed and of the ABI number expected; the same handle a second time: as it is."""
        if lib is not self._bound:
            protos = self.prototypes()
            for name in protos:
                if not hasattr(lib, name):
                    raise KbeError('%s does not export %s (stale build?)' % (self.library, name))
            bind(lib, protos)
            if self.abi is not None:
                entry, expected, label = self.abi
                if getattr(lib, entry)() != expected:
                    raise KbeError('%s %sABI %d != expected %d' % (self.library, label, getattr(lib, entry)(), expected))
            self._bound = lib
        return lib

    def raw(self, lib, name, *args):
        """The entry `name` with plain Python values -> what it returns.  ctypes holds the values to the header's types (bind); a surplus
        argument, which cdecl lets through, is refused here.  The entry is looked up on `lib` at each call (a tool may have put a shim there)."""
        proto = self.prototypes().get(name)
        if proto is None:
            raise KbeError('%s is not an entry of %s' % (name, self.name))
        if len(args) != len(proto[1]):
            raise KbeError('%s takes %d arguments, got %d' % (name, len(proto[1]), len(args)))
        return getattr(lib, name)(*args)

    @staticmethod
    def check(lib, rc, what):
        if rc != 0:
            raise KbeError('%s failed (%d): %s' % (what, rc, lib.kbe_last_error().decode()))

    def call(self, lib, name, *args, what=None):
        """An entry that returns a status: KbeError with the library's text (under the label `what`, default the entry's name) unless KBE_OK."""
        self.check(lib, self.raw(lib, name, *args), what or name)
