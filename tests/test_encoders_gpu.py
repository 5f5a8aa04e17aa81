"""The contract the device-side encoders share (include/kbe.h: kbe_mjpeg_encode, kbe_png_encode; the host side of both: csrc/kbe_units_scan.h),
once per encoder, through ctypes: streams and files against the CPU twins (tests/mjpeg_check.cpp, tests/png_check.cpp: the same block
headers compiled by g++) BYTE FOR BYTE -- the twins themselves are held against Pillow and zlib in tests/test_mjpeg_stream.py and
tests/test_png_stream.py --, the overflow contract, the argument checks and the tensor-level call.  Every case of the two CPU suites byte
for byte is encoder_gpu.assert_case's, run under each format's own test (tests/test_mjpeg_gpu.py, tests/test_png_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import encoder_gpu as eg
from encoder_gpu import SENTINEL

pytestmark = pytest.mark.gpu

each_encoder = pytest.mark.parametrize('enc', eg.ENCODERS, ids=lambda e: e.fmt)


@pytest.fixture(scope='module')
def K():
    return eg.kernels()


@each_encoder
def test_frames_that_fill_one_launch_two_launches_and_two_with_a_remainder(K, enc):
    """12, 24 and 25 frames: where the loop that cuts frames into launches of 12 ends a launch, and what it carries into the next."""
    dev = eg.on_device(enc.cases.case_frames('size_17x16', 25))
    want = enc.cases.case_twin('size_17x16', 25)[0]
    for n in (12, 24, 25):
        eg.assert_units(K, enc, dev[:n], enc.own('size_17x16') + (0,), want[:n])


@each_encoder
def test_rows_with_a_stride_and_an_unaligned_buffer(K, enc):
    frames = enc.cases.case_frames('size_50x37', 3)
    want = enc.cases.case_twin('size_50x37', 3)[0]
    own = enc.own('size_50x37') + (0,)
    wide = np.full((3, 50, 45, 3), 99, np.uint8)
    wide[:, :, :37] = frames
    eg.assert_units(K, enc, wide, own, want, room=0, W=37)
    # the buffer 1, 2 and 3 bytes off a 4-byte boundary: the stores of four bytes at a time start later
    for shift in (1, 2, 3):
        eg.assert_units(K, enc, frames, own, want, room=0, shift=shift)


@each_encoder
def test_a_buffer_too_small_reports_the_true_sizes_and_nothing_is_written_beyond_it(K, enc):
    dev = eg.on_device(enc.cases.case_frames(enc.ladder, 3))
    want = enc.cases.case_twin(enc.ladder, 3)[0]
    joined, sizes, own = b''.join(want), eg.sizes_of(want), enc.own(enc.ladder) + (0,)
    for cap in (len(joined) - 1, len(joined) - 2, sizes[1] + 5, 7, 0):          # one byte short; ...; inside the second and the first header; nothing
        rc, offsets, status, buf = eg.run(K, enc, dev, own, cap)
        assert rc == 0 and status == 1, cap
        assert offsets == sizes, cap
        assert buf[:cap].tobytes() == joined[:cap], cap                     # (what fits is the beginning)
        assert (buf[cap:] == SENTINEL).all(), cap
    rc, offsets, status, buf = eg.run(K, enc, dev, own, len(joined))            # exactly enough
    assert rc == 0 and status == 0 and buf[:len(joined)].tobytes() == joined and (buf[len(joined):] == SENTINEL).all()


@each_encoder
def test_invalid_arguments_are_refused_before_anything_is_enqueued(K, enc):
    frames = eg.on_device(enc.cases.case_frames('size_17x16', 3))
    lib, own = K.lib, enc.own('size_17x16') + (0,)

    def refused(**kw):
        rc, offsets, status, buf = eg.run(K, enc, frames, own[:-1] + (kw.pop('flags', 0),), 4096, **kw)
        return rc == -1 and status == 7 and set(offsets) == {-1} and bool((buf == SENTINEL).all())      # KBE_E_INVALID, and nothing ran
    assert refused(n=0) and refused(n=-3)
    assert refused(flags=2) and refused(flags=-1)
    assert refused(stride=3 * 16 - 1) and refused(W=0) and refused(W=17)                                    # (W = 17 > the rows' 16 pixels: stride < 3 W)
    scratch = torch.empty(4096, dtype=torch.int64, device='cuda')
    meta = torch.full((8,), -1, dtype=torch.int64, device='cuda')
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device='cuda')
    good = dict(frames=(ctypes.c_void_p * 3)(*[frames.data_ptr() + i * 17 * 16 * 3 for i in range(3)]), n=3, W=16, H=17, stride=48, own=own,
                scratch=scratch.data_ptr(), out=out.data_ptr(), cap=4096, offsets=meta.data_ptr(), status=meta.data_ptr() + 56)

    def call(**change):
        a = dict(good, **change)
        return K.encode_raw(enc.fmt, a['frames'], a['n'], a['W'], a['H'], a['stride'], a['own'], a['scratch'], a['out'], a['cap'], a['offsets'], a['status'])
    assert call(frames=None) == -1 and call(scratch=0) == -1 and call(out=0) == -1 and call(offsets=0) == -1 and call(status=0) == -1
    assert call(frames=(ctypes.c_void_p * 3)(frames.data_ptr(), None, frames.data_ptr())) == -1                # a null frame among them
    assert call(W=65536, stride=3 * 65536) == -1 and call(H=65536) == -1 and call(H=0) == -1
    assert enc.refused and all(call(**change) == -1 for change in enc.refused)                              # the entry's own: the quality; the size of a file
    assert call(scratch=scratch.data_ptr() + 4) == -1 and call(offsets=meta.data_ptr() + 4) == -1            # 8-byte alignment
    torch.cuda.synchronize()
    assert bool((meta == -1).all()) and bool((out == SENTINEL).all())
    assert ('kbe_%s_encode' % enc.fmt).encode() in lib.kbe_last_error()
    assert call() == 0                                                                                      # ... and the good call goes through
    bound, scratch_bytes = getattr(lib, 'kbe_%s_bound' % enc.fmt), getattr(lib, 'kbe_%s_scratch_bytes' % enc.fmt)
    assert int(bound(0, 5)) == 0 and int(scratch_bytes(16, 17, 0)) == 0
    assert int(scratch_bytes(1024, 1024, 75)) == int(scratch_bytes(1024, 1024, 12)) < (1 << 20)            # no worst-case stream or file in it


@each_encoder
def test_the_tensor_level_call_and_its_second_run_with_a_larger_buffer(K, enc):
    dev = eg.on_device(enc.cases.case_frames('noise', 3))
    want = enc.cases.case_twin('noise', 3)[0]
    assert enc.encode(K, dev, 'noise') == want                              # (Motion-JPEG: noise at quality 100 does not fit the first guess of a quarter of the pixels)
    assert enc.encode(K, dev, 'noise', cap=10) == want                      # the second run with the size the first reported
    assert enc.encode(K, dev, 'noise', bgr=True) == enc.cases.case_twin('noise', 3, enc.cases.BGR)[0]
    assert enc.encode(K, dev[:1], 'noise', cap=1 << 20) == want[:1]
    from ken_burns_effect_amd._native import KbeError
    with pytest.raises(KbeError):
        enc.encode(K, dev.cpu(), 'noise')
