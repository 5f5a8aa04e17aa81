"""What is PNG's own of the device-side encoder on the GPU (kbe_png_encode, include/kbe.h; kernels: csrc/kbe_png.hip): stored and coded segments
behind an unaligned start, the scan over many segments, the bound, files that decode to their frames, and the host side built on the encoder.
The contract it shares with kbe_mjpeg_encode -- byte for byte against the CPU twin, overflow, argument checks, the tensor-level call -- is
tests/test_encoders_gpu.py's."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import encoder_gpu as eg
import png_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    return eg.kernels()


@pytest.fixture(scope='module')
def rendered(K):
    return eg.rendered(K)


@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_device_files_are_the_twins_byte_for_byte(K, name):
    eg.assert_case(K, eg.PNG, name)


def test_an_unaligned_buffer_with_stored_segments_and_coded_ones_of_more_than_one_store_per_lane(K):
    for name in ('noise', 'photo_like'):
        eg.assert_units(K, eg.PNG, pc.case_frames(name, 3), (pc.BGR,), pc.case_twin(name, 3, pc.BGR)[0], room=0, shift=3)


def test_the_scan_over_many_segments(K):
    """More segments than one workgroup of the scan takes (256) in one frame; the scan itself is the one kbe_mjpeg_encode uses
    (csrc/kbe_units_scan.h), whose second level tests/test_mjpeg_gpu.py reaches."""
    frames = eg.tiled(1200, 1200, 11)[None]
    want, _, segment, _ = pc.twin(frames)
    assert -(-1200 * 3601 // segment) > 256
    eg.assert_units(K, eg.PNG, frames, (0,), want)


def test_the_bound_is_the_twins_noise_reaches_it_and_it_refuses_files_of_2_to_the_31(K):
    noisy = pc.case_twin('noise', 3)
    assert int(K.lib.kbe_png_bound(80, 100)) == noisy[3] == len(noisy[0][0])
    assert int(K.lib.kbe_png_bound(65535, 65535)) == 0 and int(K.lib.kbe_png_bound(30000, 24000)) == 0 and 0 < int(K.lib.kbe_png_bound(30000, 23000)) < 2 ** 31


def test_the_tensor_level_calls_files_decode_to_their_frames(K):
    frames = pc.case_frames('noise', 3)
    for data, frame in zip(K.png_encode(eg.on_device(frames)), frames):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), frame)


@pytest.mark.parametrize('pretrained_estim', [False, True], ids=['bgr', 'rgb'])
@pytest.mark.parametrize('jpeg', ['native', 'device'])
def test_the_pipeline_writes_its_png_frames_from_hbm_under_the_switch(K, rendered, pretrained_estim, jpeg, monkeypatch, tmp_path):
    """Pipeline._run with KBE_PNG=device and PNG frames asked for: the frame loop is asked to leave its frames on the device, each is
    encoded once, frames/%d.png decode to the frames in RGB, the video is still written, and the frames come back as numpy arrays."""
    from ken_burns_effect_amd import pipeline as P
    in_hbm, raw = rendered
    Stub, asked = eg.pipeline_without_models(P, monkeypatch, in_hbm, raw)
    monkeypatch.setenv('KBE_PNG', 'device')
    monkeypatch.setenv('KBE_JPEG', jpeg)
    image = torch.zeros(1, 3, 96, 128)
    out = Stub(True)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is True
    assert len(out) == 2 and all(isinstance(f, np.ndarray) and np.array_equal(f, r) for f, r in zip(out, raw))
    want = pc.twin(raw, 0 if pretrained_estim else pc.BGR)[0]
    for i in range(2):
        data = open(str(tmp_path / 'frames' / ('%d.png' % i)), 'rb').read()
        assert data == want[i]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), raw[i] if pretrained_estim else raw[i][:, :, ::-1])
    assert not (tmp_path / 'frames' / '2.png').exists()
    video = open(str(tmp_path / '3d_kbe.mp4'), 'rb').read()
    assert video.count(b'\xff\xd8\xff\xe0') == 3                            # forth and back: three Motion-JPEG frames
    # no PNG frames asked for: the switch changes nothing
    monkeypatch.setenv('KBE_JPEG', 'native')
    Stub(False)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path / 'plain'), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is False and not (tmp_path / 'plain' / 'frames').exists()
    # without the switch: today's host route, today's files
    monkeypatch.delenv('KBE_PNG')
    Stub(True)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path / 'host'), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is False
    rgb = raw[1] if pretrained_estim else raw[1][:, :, ::-1]
    assert open(str(tmp_path / 'host' / 'frames' / '1.png'), 'rb').read() == P.png_bytes(rgb)


def test_one_idat_that_zlib_inflates_to_the_filtered_bytes(K):
    frame = pc.case_frames('size_17x16', 1)
    data = K.png_encode(torch.from_numpy(np.ascontiguousarray(frame)).cuda())[0]
    idat = [body for tag, body in pc.chunks(data) if tag == b'IDAT']
    assert len(idat) == 1 and zlib.decompress(idat[0]) == pc.filtered(frame[0])
