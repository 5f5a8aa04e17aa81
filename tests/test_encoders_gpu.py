"""The contract the device-side encoders share (kbe_mjpeg_encode and kbe_png_encode of include/kbe.h, kbe_gif_encode of include/kbe_gif.h; the host
side of all three: csrc/kbe_units_scan.h), once per encoder, through the typed bindings: streams, files and units against the CPU twins
(tests/mjpeg_check.cpp, png_check.cpp, gif_check.cpp: the same block headers compiled by g++) BYTE FOR BYTE -- the twins themselves are held
against Pillow and zlib in tests/test_mjpeg_stream.py, test_png_stream.py and test_gif_stream.py --, the overflow contract, the argument checks,
one test per refusal, and the tensor-level call.  Every case of the three CPU suites byte for byte is encoder_gpu.assert_case's, run under each
format's own test (tests/test_mjpeg_gpu.py, test_png_gpu.py, test_gif_gpu.py)."""
import numpy as np
import pytest

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
    name = enc.sized % '17x16'
    dev = eg.on_device(enc.cases.case_frames(name, 25))
    want = enc.cases.case_twin(name, 25)[0]
    for n in (12, 24, 25):
        eg.assert_units(K, enc, dev[:n], enc.own(name), want[:n])


@each_encoder
def test_rows_with_a_stride_and_an_unaligned_buffer(K, enc):
    name = enc.sized % '50x37'
    frames = enc.cases.case_frames(name, 3)
    want = enc.cases.case_twin(name, 3)[0]
    wide = np.full((3, 50, 45, 3), 99, np.uint8)
    wide[:, :, :37] = frames
    eg.assert_units(K, enc, wide, enc.own(name), want, room=0, W=37)
    # the buffer 1, 2 and 3 bytes off a 4-byte boundary: the stores of four bytes at a time start later
    for shift in (1, 2, 3):
        eg.assert_units(K, enc, frames, enc.own(name), want, room=0, shift=shift)


@each_encoder
def test_a_buffer_too_small_reports_the_true_sizes_and_nothing_is_written_beyond_it(K, enc):
    """status 1, the true offsets, the twin's bytes below cap and nothing at or beyond it; the rerun at offsets[n] succeeds."""
    dev = eg.on_device(enc.cases.case_frames(enc.ladder, 3))
    want = enc.cases.case_twin(enc.ladder, 3)[0]
    joined, sizes, own = b''.join(want), eg.sizes_of(want), enc.own(enc.ladder)
    total = len(joined)
    for cap in (0, 1, 7, sizes[1] - 1, sizes[1] + 5, sizes[2] - 1, total - 2, total - 1):     # nothing; inside the first header; ...; inside the second; ...; one byte short
        rc, offsets, status, buf, _ = eg.run(K, enc, dev, own, cap)
        assert rc == 0 and status == 1, cap
        assert offsets == sizes, cap
        assert buf[:cap].tobytes() == joined[:cap], cap                     # (what fits is the beginning)
        assert (buf[cap:] == SENTINEL).all(), cap
    rc, offsets, status, buf, _ = eg.run(K, enc, dev, own, offsets[3])          # exactly enough: what the run before reported
    assert rc == 0 and status == 0 and offsets[3] == total and buf[:total].tobytes() == joined and (buf[total:] == SENTINEL).all()
    # out may be NULL when cap is 0
    rc, offsets, status, _, _ = eg.run(K, enc, dev, own, 0, change=lambda a: a.update(out=None))
    assert rc == 0 and status == 1 and offsets == sizes


# (the GIF's refusals run under the ids they have had from the start: tests/test_gif_gpu.py::test_refusals_leave_every_buffer_untouched)
@pytest.mark.parametrize('enc, what', [(enc, what) for enc in (eg.MJPEG, eg.PNG) for what in eg.refusals_of(enc)], ids=lambda v: getattr(v, 'fmt', v))
def test_a_refusal_leaves_every_buffer_untouched(K, enc, what):
    eg.assert_refused(K, enc, what)


@each_encoder
def test_the_good_call_goes_through_and_the_sizes_refuse_what_the_entry_refuses(K, enc):
    name = enc.sized % '17x16'
    want = enc.cases.case_twin(name, 3)[0]
    rc, offsets, status, buf, _ = eg.run(K, enc, eg.on_device(enc.cases.case_frames(name, 3)), enc.own(name), 4096)     # the refusals' call, unchanged
    assert rc == 0 and status == 0 and offsets == eg.sizes_of(want) and buf[:offsets[3]].tobytes() == b''.join(want)
    lib = enc.via(K)[1]
    bound, scratch_bytes = getattr(lib, 'kbe_%s_bound' % enc.fmt), getattr(lib, 'kbe_%s_scratch_bytes' % enc.fmt)
    assert int(bound(0, 5)) == 0 and int(scratch_bytes(16, 17, 0)) == 0
    assert int(scratch_bytes(1024, 1024, 75)) == int(scratch_bytes(1024, 1024, 12)) < (1 << 20)            # no worst-case stream, file or unit in it


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
