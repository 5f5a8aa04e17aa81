"""The stream of the device-side Motion-JPEG encoder, on the CPU: ken-burns-effect_amd/csrc/kbe_mjpeg_block.h -- the one definition of
its arithmetic and format, which hipcc compiles into the kernels of kbe_mjpeg.hip -- compiled by g++ into tests/mjpeg_check.cpp and
executed serially (tests/test_mjpeg_gpu.py holds the device to these very bytes).  Pillow is the CHECKER, the bars are those of
tests/test_jpeg_writer.py: Pillow's tables, 0.5 dB, 5 % + 64 bytes; the one addition to that stream are restart intervals."""
import io

import numpy as np
import pytest
from PIL import Image

import mjpeg_cases as mc
from test_jpeg_writer import decode, pillow, psnr, tables


def pillow_with_restarts(frame, quality, R):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame)).save(buf, format='JPEG', quality=quality, restart_marker_blocks=R)
    return buf.getvalue()


@pytest.mark.parametrize('quality', mc.QUALITIES)
def test_tables_are_pillows_and_restart_markers_cycle(quality):
    name = 'quality_%d' % quality
    frame = mc.case_frames(name)[0]
    (mine,), _, R, _ = mc.case_twin(name)
    q_mine, h_mine, sof_mine = tables(mine)
    q_pil, h_pil, sof_pil = tables(pillow(frame, quality))
    assert q_mine == q_pil and set(q_mine) == {0, 1}
    assert h_mine == h_pil and set(h_mine) == {0x00, 0x10, 0x01, 0x11}
    assert sof_mine == sof_pil
    declared, markers = mc.restart_interval(mine)
    assert declared == R and 1 <= R <= 8
    mcus = -(-frame.shape[0] // 16) * -(-frame.shape[1] // 16)
    assert len(markers) == -(-mcus // R) - 1 and markers == [i & 7 for i in range(len(markers))]
    assert mine[:2] == b'\xff\xd8' and mine[-2:] == b'\xff\xd9'


@pytest.mark.parametrize('size', mc.SIZES)
def test_streams_decode_to_the_picture_as_well_as_pillows_do(size):
    h, w = size
    name = 'size_%dx%d' % size
    frame = mc.case_frames(name)[0]
    (mine,), _, R, bound = mc.case_twin(name)
    assert mine[:2] == b'\xff\xd8' and mine[-2:] == b'\xff\xd9' and len(mine) <= bound
    got = decode(mine)
    assert got.shape == (h, w, 3)
    ours, theirs = psnr(got, frame), psnr(decode(pillow(frame, 92)), frame)
    print('%dx%d: twin %.2f dB, Pillow %.2f dB; %d bytes, Pillow with R = %d: %d' % (h, w, ours, theirs, len(mine), R, len(pillow_with_restarts(frame, 92, R))))
    assert ours > theirs - 0.5
    if h * w >= 1000:
        assert abs(len(mine) - len(pillow_with_restarts(frame, 92, R))) < 0.05 * len(mine) + 64
    declared, markers = mc.restart_interval(mine)
    mcus = -(-h // 16) * -(-w // 16)
    assert declared == R and markers == [i & 7 for i in range(-(-mcus // R) - 1)]


def test_restart_intervals_do_not_change_the_picture():
    """What Pillow decodes from Pillow's own stream with and without restart intervals is the same picture: the intervals cost bytes, not quality."""
    frame = mc.case_frames('size_96x128')[0]
    R = mc.case_twin('size_96x128')[2]
    assert np.array_equal(decode(pillow_with_restarts(frame, 92, R)), decode(pillow(frame, 92)))


@pytest.mark.parametrize('name', ['size_50x37', 'noise', 'rst_wrap'])
def test_bgr_frames_under_the_flag_give_the_rgb_bytes(name):
    frames = mc.case_frames(name)
    swapped = np.ascontiguousarray(frames[..., ::-1])
    assert mc.twin(swapped, mc.CASES[name][2], mc.BGR)[0] == mc.case_twin(name)[0]
    assert mc.twin(swapped, mc.CASES[name][2], 0)[0] != mc.case_twin(name)[0]


def test_inputs_that_reach_the_rare_paths():
    """Every branch of the entropy coder is taken by some case (the counters are the twin's own: kbe_mjpeg_block.h's Stats), and what
    comes out still decodes to the picture."""
    streams, stats, _, bound = mc.case_twin('noise')
    print('noise', stats)
    assert stats['stuffed'] > 0 and stats['noeob'] > 0 and len(streams[0]) <= bound
    frame = mc.case_frames('noise')[0]
    assert psnr(decode(streams[0]), frame) > psnr(decode(pillow(frame, 100)), frame) - 0.5
    streams, stats, _, _ = mc.case_twin('checkerboard')
    print('checkerboard', stats)
    assert stats['dc11'] > 0
    assert np.abs(decode(streams[0]).astype(int) - mc.case_frames('checkerboard')[0]).max() <= 2
    streams, stats, _, _ = mc.case_twin('speck')
    print('speck', stats)
    assert stats['zrl'] > 0
    frame = mc.case_frames('speck')[0]
    assert psnr(decode(streams[0]), frame) > psnr(decode(pillow(frame, 50)), frame) - 0.5
    streams, stats, R, _ = mc.case_twin('rst_wrap')
    print('rst_wrap', stats)
    declared, markers = mc.restart_interval(streams[0])
    assert stats['rstwrap'] > 0 and len(markers) > 8 and markers[8] == 0 and (R == 1 or 71 % R != 0)


@pytest.mark.parametrize('name', ['size_50x37', 'noise', 'checkerboard', 'speck', 'rst_wrap', 'quality_10', 'widest', 'tallest'])
def test_blocks_coded_on_their_own_and_joined_give_the_same_bytes(name):
    """The kernels code the blocks of an interval side by side -- each block's bits packed into words of their own -- and join them
    afterwards: the same functions in that order on the CPU give the stream of the straight run, counters included."""
    streams, stats, _, _ = mc.twin(mc.case_frames(name, 2), mc.CASES[name][2], packed=True)
    want, want_stats, _, _ = mc.case_twin(name, 2)
    assert streams == want and stats == want_stats


def test_flat_frames():
    for value in (0, 255, 128):
        flat = np.full((1, 40, 40, 3), value, np.uint8)
        assert np.abs(decode(mc.twin(flat, 92)[0][0]).astype(int) - value).max() <= 1


@pytest.mark.parametrize('container', ['mp4', 'avi'])
def test_the_writers_take_streams_that_are_encoded_already(container, monkeypatch, tmp_path):
    from ken_burns_effect_amd import pipeline
    frames = mc.case_frames('size_96x128', 3)
    video = [frames[0], frames[1], frames[2], frames[1], frames[0]]
    encoded = mc.case_twin('size_96x128', 3)[0]
    jpegs = [encoded[i] for i in (0, 1, 2, 1, 0)]
    writer = pipeline.write_mjpeg_mp4 if container == 'mp4' else pipeline.write_mjpeg_avi
    given = writer(str(tmp_path / ('given.' + container)), None, fps=25, jpegs=jpegs, frame_size=(96, 128))
    monkeypatch.setattr(pipeline, '_jpegs', lambda frames_rgb, quality: jpegs)
    from_frames = writer(str(tmp_path / ('frames.' + container)), video, fps=25)
    assert open(given, 'rb').read() == open(from_frames, 'rb').read()
    monkeypatch.setattr(pipeline.shutil, 'which', lambda name: None)
    assert pipeline.write_video(str(tmp_path / ('video.' + container)), None, fps=25, jpegs=jpegs, frame_size=(96, 128)) is False
    assert open(str(tmp_path / ('video.' + container)), 'rb').read() == open(given, 'rb').read()
    with pytest.raises(ValueError):
        writer(str(tmp_path / 'x'), None, jpegs=jpegs)                  # streams without the frame size


def test_the_switch_and_the_command_line():
    from ken_burns_effect_amd import kbe
    assert kbe.parse(['--jpeg', 'device'])[0]['jpeg'] == 'device' and kbe.parse([])[0]['jpeg'] is None
