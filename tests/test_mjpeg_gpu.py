"""What is Motion-JPEG's own of the device-side encoder on the GPU (kbe_mjpeg_encode, include/kbe.h; kernels: csrc/kbe_mjpeg.hip): the scan over many
restart intervals, the bound, the picture's quality, and the host side built on the encoder.  The contract it shares with kbe_png_encode --
byte for byte against the CPU twin, overflow, argument checks, the tensor-level call -- is tests/test_encoders_gpu.py's."""
import numpy as np
import pytest
import torch

import encoder_gpu as eg
import mjpeg_cases as mc
from test_jpeg_writer import decode, pillow, psnr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    return eg.kernels()


@pytest.fixture(scope='module')
def rendered(K):
    return eg.rendered(K)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_device_streams_are_the_twins_byte_for_byte(K, name):
    eg.assert_case(K, eg.MJPEG, name)


@pytest.mark.parametrize('shape', [(3, 512, 768), (1, 4096, 4112)], ids=['1152_intervals', '16448_intervals'])
def test_the_scan_over_many_intervals(K, shape):
    """More intervals than one workgroup of the scan takes (256), and more sums of 256 than the scan of the sums takes at once (64)."""
    n, h, w = shape
    frames = np.stack([eg.tiled(h, w, 11 + i) for i in range(n)])
    want, _, R, _ = mc.twin(frames, 75)
    assert n * -(-(-(-h // 16) * -(-w // 16)) // R) > (256 if n == 3 else 64 * 256)
    eg.assert_units(K, eg.MJPEG, frames, (75, 0), want)


def test_the_bound_is_the_twins_and_holds_noise(K):
    streams, _, _, bound = mc.case_twin('noise', 3)
    assert sum(len(s) for s in streams) <= 3 * int(K.lib.kbe_mjpeg_bound(80, 64)) and int(K.lib.kbe_mjpeg_bound(80, 64)) == bound


def test_rendered_frames_encoded_where_they_lie_decode_to_the_frames_delivered_raw(K, rendered):
    in_hbm, raw = rendered
    assert in_hbm.is_cuda and raw.shape == (2, 96, 128, 3)
    streams = K.mjpeg_encode(in_hbm, 92)
    assert streams == mc.twin(raw, 92)[0]
    for stream, frame in zip(streams, raw):
        got = decode(stream)
        ours, theirs = psnr(got, frame), psnr(decode(pillow(frame, 92)), frame)
        print('device %.2f dB, Pillow %.2f dB' % (ours, theirs))
        assert got.shape == frame.shape and ours > theirs - 0.5


def test_write_video_under_the_switch_holds_the_device_streams(K, rendered, monkeypatch, tmp_path):
    from ken_burns_effect_amd import pipeline
    _, raw = rendered
    monkeypatch.setenv('KBE_JPEG', 'device')
    monkeypatch.setattr(pipeline.shutil, 'which', lambda name: None)
    assert pipeline.jpeg_encoder()[0] == 'device'
    frames = [raw[0], raw[1]]
    assert pipeline.write_video(str(tmp_path / 'v.mp4'), frames + frames[-2::-1], fps=25) is False
    want = mc.twin(raw, 92)[0]
    data = open(str(tmp_path / 'v.mp4'), 'rb').read()
    assert want[0] + want[1] + want[0] in data and data.count(b'\xff\xd8\xff\xe0') == 3
    monkeypatch.delenv('KBE_JPEG')
    assert pipeline.jpeg_encoder()[0] == 'native'                           # the default stays


@pytest.mark.parametrize('pretrained_estim', [False, True], ids=['bgr', 'rgb'])
def test_the_pipeline_keeps_its_frames_in_hbm_under_the_switch(K, rendered, pretrained_estim, monkeypatch, tmp_path):
    """Pipeline._run with KBE_JPEG=device, no ffmpeg and no PNG frames: the frame loop is asked to leave its frames on the device, each is
    encoded once (in the input's channel order), the video goes forth and back, and the frames come back as numpy arrays all the same."""
    from ken_burns_effect_amd import pipeline as P
    in_hbm, raw = rendered
    Stub, asked = eg.pipeline_without_models(P, monkeypatch, in_hbm, raw)
    monkeypatch.setenv('KBE_JPEG', 'device')
    image = torch.zeros(1, 3, 96, 128)
    out = Stub(False)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is True
    assert len(out) == 2 and all(isinstance(f, np.ndarray) and np.array_equal(f, r) for f, r in zip(out, raw))
    want = mc.twin(raw, 92, 0 if pretrained_estim else mc.BGR)[0]
    data = open(str(tmp_path / '3d_kbe.mp4'), 'rb').read()
    assert want[0] + want[1] + want[0] in data
    # PNG frames asked for: today's route, whatever the switch says
    Stub(True)(image, {'objectFrom': {}, 'objectTo': {}}, str(tmp_path / 'png'), pretrained_estim=pretrained_estim)
    assert asked['keep_on_device'] is False and (tmp_path / 'png' / 'frames' / '1.png').exists()
