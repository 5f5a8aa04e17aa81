"""What a caller of the device-side encoders (kbe_mjpeg_encode, kbe_png_encode: include/kbe.h) sees without a GPU: the sizes it allocates
by, and every refusal with its text.  A refusal returns before anything is enqueued, so host memory stands in for every pointer; no call
here has valid arguments (those belong to tests/test_encoders_gpu.py)."""
import ctypes

import pytest

SIZES = [   # W, H, n, mjpeg scratch, png scratch, mjpeg bound, png bound
    (16, 17, 3, 48, 84, 5627, 903),
    (37, 50, 13, 440, 296, 30595, 5670),
    (128, 96, 2, 296, 152, 120487, 37040),
    (1200, 1200, 1, 16936, 6352, 14046259, 4322585),
    (1024, 1024, 12, 147840, 55664, 10228343, 3147782),
    (1024, 1024, 75, 147840, 55664, 10228343, 3147782),
    (4112, 4096, 1, 197896, 74148, 164283255, 50547842),
]
OWN = {'kbe_mjpeg_encode': 'bad stride, quality or flags', 'kbe_png_encode': 'bad stride or flags'}


@pytest.fixture(scope='module')
def lib():
    from ken_burns_effect_amd import _native
    return _native.load()


@pytest.mark.parametrize('row', SIZES, ids=lambda r: '%dx%dx%d' % r[:3])
def test_the_sizes_callers_allocate_by(lib, row):
    W, H, n, mjpeg_scratch, png_scratch, mjpeg_bound, png_bound = row
    assert lib.kbe_mjpeg_scratch_bytes(W, H, n) == mjpeg_scratch and lib.kbe_png_scratch_bytes(W, H, n) == png_scratch
    assert lib.kbe_mjpeg_bound(W, H) == mjpeg_bound and lib.kbe_png_bound(W, H) == png_bound


def test_the_sizes_of_what_is_refused_are_zero(lib):
    for bound, scratch in ((lib.kbe_mjpeg_bound, lib.kbe_mjpeg_scratch_bytes), (lib.kbe_png_bound, lib.kbe_png_scratch_bytes)):
        assert bound(0, 5) == 0 and scratch(16, 17, 0) == 0
    assert lib.kbe_png_bound(65535, 65535) == 0 and lib.kbe_png_bound(30000, 24000) == 0
    assert 0 < lib.kbe_png_bound(30000, 23000) < 2 ** 31


@pytest.mark.parametrize('entry', sorted(OWN))
def test_every_refusal_and_its_text(lib, entry):
    memory = (ctypes.c_uint64 * 1024)()                                     # host memory, 8-byte aligned: nothing reads or writes it
    at = ctypes.addressof(memory)
    good = dict(frames=(ctypes.c_void_p * 3)(at + 4096, at + 4096, at + 4096), n=3, W=16, H=17, stride=48, quality=92, flags=0, scratch=at, out=at + 1024, cap=1024,
                offsets=at + 2048, status=at + 3072)

    def refused(what, **change):
        a = dict(good, **change)
        own = [ctypes.c_int(a['quality'])] if entry == 'kbe_mjpeg_encode' else []
        rc = getattr(lib, entry)(a['frames'], ctypes.c_int(a['n']), ctypes.c_int(a['W']), ctypes.c_int(a['H']), ctypes.c_int(a['stride']), *own, ctypes.c_int(a['flags']),
                                 ctypes.c_void_p(a['scratch']), ctypes.c_void_p(a['out']), ctypes.c_size_t(a['cap']), ctypes.c_void_p(a['offsets']), ctypes.c_void_p(a['status']), None)
        assert (rc, lib.kbe_last_error().decode()) == (-1, '%s: %s' % (entry, what)), change
    for change in (dict(n=0), dict(n=-3), dict(W=0), dict(H=0), dict(H=65536), dict(W=65536, stride=3 * 65536), dict(frames=None)):
        refused('bad frames or size', **change)
    for change in (dict(flags=2), dict(flags=-1), dict(stride=3 * 16 - 1)) + ((dict(quality=0), dict(quality=101)) if entry == 'kbe_mjpeg_encode' else ()):
        refused(OWN[entry], **change)
    if entry == 'kbe_png_encode':
        refused("a frame's file would not stay below 2^31 bytes", W=65535, H=65535, stride=3 * 65535)
    for change in (dict(scratch=None), dict(offsets=None), dict(status=None), dict(scratch=at + 4), dict(offsets=at + 2052), dict(out=None)):
        refused('bad buffers', **change)
    refused('null frame', frames=(ctypes.c_void_p * 3)(at + 4096, None, at + 4096))
