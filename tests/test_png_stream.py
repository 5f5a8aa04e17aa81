"""The PNG file of the device-side frame writer (csrc/kbe_png_block.h, include/kbe.h: kbe_png_encode), on the CPU: the header compiled by g++
and executed serially (tests/png_check.cpp) writes files that Pillow opens to the frame's own bytes, whose one IDAT zlib inflates to the
filtered bytes pipeline.png_bytes compresses, and whose lengths and check sums are zlib's; the code construction on its own; the sizes
against today's files; and the host side of the switch.  tests/test_png_gpu.py holds the kernels against these files byte for byte."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as pc

GOLDEN = os.path.join(pc.ROOT, 'tests', 'golden')


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


@pytest.mark.parametrize('flags', [0, pc.BGR], ids=['rgb', 'bgr'])
@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_the_twins_file_is_a_png_of_the_frame(name, flags):
    frames = pc.case_frames(name, 3)
    files, stats, segment, bound = pc.case_twin(name, 3, flags)
    assert segment == pc.SEGMENT
    for data, frame in zip(files, frames):
        rgb = frame[:, :, ::-1] if flags else frame
        parts = pc.chunks(data)                                             # (lengths and CRCs against zlib.crc32)
        assert [tag for tag, _ in parts] == [b'IHDR', b'IDAT', b'IEND']     # exactly one IDAT
        h, w = frame.shape[:2]
        assert parts[0][1] == struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0) and parts[2][1] == b''
        idat = parts[1][1]
        assert idat[:2] == b'\x78\x01'
        raw = zlib.decompress(idat)
        assert raw == pc.filtered(rgb)
        assert idat[-4:] == struct.pack('>I', zlib.adler32(raw) & 0xFFFFFFFF) and idat[-6:-4] == b'\x03\x00'
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), rgb)
        assert len(data) <= bound
    segments = -(-len(pc.filtered(frames[0])) // segment)
    assert stats['coded'] + stats['stored'] == 3 * segments
    assert bound == 43 + 22 + len(pc.filtered(frames[0])) + 5 * segments


@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_the_kernels_steps_give_the_same_bytes(name):
    """A segment in pieces of 64 bytes that learn from their neighbours where runs start, every piece's bits packed at their place."""
    assert pc.twin(pc.case_frames(name, 3), pc.BGR, pieces=True)[0] == pc.case_twin(name, 3, pc.BGR)[0]


def test_what_the_cases_are_there_for():
    one = pc.case_twin('one_segment', 3)
    assert len(pc.filtered(pc.case_frames('one_segment')[0])) == pc.SEGMENT and one[1]['coded'] + one[1]['stored'] == 3
    past = pc.case_twin('one_past_segment', 3)
    assert len(pc.filtered(pc.case_frames('one_past_segment')[0])) == pc.SEGMENT + 1 and past[1]['coded'] + past[1]['stored'] == 6
    assert past[1]['stored'] >= 3                                           # (a segment of one byte leaves stored)
    noisy = pc.case_twin('noise', 3)
    assert noisy[1]['coded'] == 0 and all(len(f) == noisy[3] for f in noisy[0])        # every segment stored: the bound is reached
    assert pc.case_twin('fibonacci', 3)[1]['limited_lit'] == 3              # the 15-bit limit cut the literal/length code of every frame
    flat = pc.case_twin('flat', 3)
    assert flat[1]['stored'] == 0 and all(len(f) < 400 for f in flat[0])    # 36 040 filtered bytes: chains of 258-byte matches
    # stripes: runs of 2, 3, 4, 258 .. 261 are in the filtered bytes
    raw = np.frombuffer(pc.filtered(pc.case_frames('stripes')[0]), np.uint8)
    edges = np.flatnonzero(np.diff(raw) != 0)
    assert {2, 3, 4, 258, 259, 260, 261} <= set(np.diff(edges).tolist())


@pytest.mark.parametrize('limit,histogram,cut', [(15, fib(30), 1), (7, fib(19), 1), (15, [7] * 286, 0), (7, [1] * 19, 0), (15, [3, 0, 5], 0), (15, [1] + [0] * 200 + [4000], 0),
                                                 (15, [1, 1] + [1000] * 255, 0)],
                         ids=['fibonacci_15', 'fibonacci_7', 'all_286_equal', 'all_19_equal', 'two_used', 'two_used_far_apart', 'two_rare'])
def test_code_lengths_stay_within_the_limit_and_are_complete(limit, histogram, cut):
    lengths, limited, kraft, whole = pc.code_lengths(limit, histogram)
    assert len(lengths) == len(histogram)
    assert all((n > 0) == (l > 0) for n, l in zip(histogram, lengths)) and max(lengths) <= limit
    assert kraft == whole                                                   # the Kraft sum is exactly 1
    assert limited == cut                                                   # (Fibonacci counts: the tree is as deep as the symbols are many)
    # rarer symbols never get shorter codes
    used = sorted((n, l) for n, l in zip(histogram, lengths) if n)
    assert all(a[1] >= b[1] for a, b in zip(used, used[1:]) if a[0] < b[0])


def test_a_single_used_symbol_gets_one_bit():
    """The one code that is not complete (Kraft sum 1/2): the convention of the format for a code of one symbol."""
    lengths, limited, kraft, whole = pc.code_lengths(15, [0, 0, 9, 0])
    assert lengths == [0, 0, 1, 0] and limited == 0 and 2 * kraft == whole


def test_unlimited_fibonacci_codes_are_what_huffman_gives():
    lengths, limited, _, _ = pc.code_lengths(15, fib(15))
    assert limited == 0 and lengths == [14, 14] + list(range(13, 0, -1))


def photographs():
    from test_jpeg_writer import photo_like
    yield 'photo_like_512', photo_like(512, 512, 3)
    for name in ('kenburns_at_size_kbe_photo.npz', 'kenburns_at_size_dolly_photo.npz'):
        frames = np.load(os.path.join(GOLDEN, name))['frames']
        yield name, frames[len(frames) // 2]


def test_photographs_are_no_larger_than_todays_files():
    from ken_burns_effect_amd import pipeline
    for name, frame in photographs():
        ours, theirs = len(pc.twin(frame[None])[0][0]), len(pipeline.png_bytes(frame))
        print('%s: %d bytes, png_bytes %d: %.3f' % (name, ours, theirs, ours / theirs))
        assert ours <= theirs, name


def test_the_ratios_of_all_cases(capsys):
    """(printed for DESIGN.md; asserted: no case beyond the bound)"""
    from ken_burns_effect_amd import pipeline
    for name in sorted(pc.CASES):
        frame = pc.case_frames(name)[0]
        files, _, _, bound = pc.case_twin(name, 1)
        with capsys.disabled():
            print('%-18s %6d bytes, png_bytes %6d: %.3f' % (name, len(files[0]), len(pipeline.png_bytes(frame)), len(files[0]) / len(pipeline.png_bytes(frame))))
        assert len(files[0]) <= bound


def test_write_frames_writes_pre_encoded_files(tmp_path):
    from ken_burns_effect_amd import pipeline
    pipeline.write_frames(str(tmp_path / 'a'), None, pngs=[b'first', b'second', b'third'])
    assert [open(str(tmp_path / 'a' / ('%d.png' % i)), 'rb').read() for i in range(3)] == [b'first', b'second', b'third']
    frame = pc.case_frames('size_17x16')[0]
    pipeline.write_frames(str(tmp_path / 'b'), [frame])                     # without them: today's files
    assert open(str(tmp_path / 'b' / '0.png'), 'rb').read() == pipeline.png_bytes(frame)


def test_the_switch(monkeypatch):
    from ken_burns_effect_amd import kbe, pipeline
    monkeypatch.delenv('KBE_PNG', raising=False)
    assert pipeline.png_encoder() == 'native'
    monkeypatch.setenv('KBE_PNG', 'device')
    assert pipeline.png_encoder() == 'device'
    monkeypatch.setenv('KBE_PNG', 'native')
    assert pipeline.png_encoder() == 'native'
    monkeypatch.setenv('KBE_PNG', 'gpu')
    with pytest.raises(ValueError):
        pipeline.png_encoder()
    assert kbe.parse(['--png', 'device'])[0]['png'] == 'device' and kbe.parse(['--png', 'native'])[0]['png'] == 'native' and kbe.parse([])[0]['png'] is None
    with pytest.raises(SystemExit):
        kbe.parse(['--png', 'fast'])


def test_the_library_and_the_bindings_know_abi_13():
    from ken_burns_effect_amd import _native
    header = open(os.path.join(pc.ROOT, 'include', 'kbe.h')).read()
    assert '#define KBE_ABI_VERSION 13' in header and _native.ABI_VERSION == 13 and _native.KBE_PNG_BGR == 1
    assert {'kbe_png_bound', 'kbe_png_scratch_bytes', 'kbe_png_encode'} <= set(_native.SYMBOLS)
    lib = _native.load()
    assert int(lib.kbe_png_bound(80, 100)) == pc.case_twin('noise', 3)[3] and int(lib.kbe_png_bound(65535, 65535)) == 0
