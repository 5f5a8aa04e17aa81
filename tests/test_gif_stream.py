"""The animated GIF of the device-side encoder on the CPU: the twin (tests/gif_check.cpp: csrc/kbe_gif_block.h compiled by g++) against Pillow's
decoder and against a reader of this suite's own, the stream's structure, the bound, the palette, and the host side of gif.py with the
device calls replaced by the twin and the NumPy restatements.  No GPU."""
import functools
import io

import numpy as np
import pytest
from PIL import Image

import gif_cases as gc


@pytest.fixture(scope='module')
def gif():
    from ken_burns_effect_amd import gif as module
    return module


def decoded(data):
    im = Image.open(io.BytesIO(data))
    frames = []
    for i in range(im.n_frames):
        im.seek(i)
        frames.append(np.asarray(im.convert('RGB')))
    return im, frames


@functools.lru_cache(maxsize=None)
def WIDTHS():
    """{k: (code_width(k), bits_before(k))} of the header, for every k a segment can have."""
    return gc.twin_widths(range(gc.SEGMENT + 1))


def segments_of(codes):
    """The code list of a frame cut at its runs of Clears: [(data codes, the closing code, the 9-bit Clears behind it)]."""
    assert codes[0][0] == 256 and codes[0][1:] == (9, 0), 'a frame starts with a Clear of 9 bits'
    out, data, i = [], [], 1
    while i < len(codes):
        code = codes[i]
        i += 1
        if code[0] < 256 or code[0] > 257:
            data.append(code)
            continue
        pads = []
        while code[0] == 256 and i < len(codes) and codes[i][0] == 256:
            pads.append(codes[i])
            i += 1
        out.append((data, code, pads))
        data = []
    assert not data and out[-1][1][0] == 257
    return out


@pytest.mark.parametrize('dither', [0, gc.DITHER], ids=['plain', 'dithered'])
@pytest.mark.parametrize('flags', [0, gc.BGR], ids=['rgb', 'bgr'])
@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_pillow_decodes_the_twins_file_to_the_intended_pixels(gif, name, flags, dither):
    frames = gc.case_frames(name, 2)
    palette, table = gc.case_palette(name, flags)
    units, stats, segment, bound = gc.case_twin(name, 2, flags, dither)
    h, w = frames.shape[1:3]
    assert segment == gc.SEGMENT and all(len(u) <= bound for u in units)
    data = gif.assemble(units, w, h, palette)
    im, got = decoded(data)
    assert im.n_frames == 2 and im.size == (w, h) and im.info['loop'] == 0 and im.info['duration'] == 40
    for frame, mine in zip(frames, got):
        assert np.array_equal(mine, palette[table[gc.cells(frame, bool(flags), dither)]])


@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_the_readers_view_of_the_stream(gif, name):
    """Every segment ends on a byte boundary and at the end of a sub-block, takes kSegmentPixels pixels (the last one the rest), is padded by at
    most 7 Clears, and every code has the width of the header's closed form; the reader itself asserts that no code exceeds the table and
    that the table never fills."""
    frames = gc.case_frames(name, 1)
    palette, table = gc.case_palette(name)
    h, w = frames.shape[1:3]
    units, stats, _, _ = gc.case_twin(name, 1, 0, gc.DITHER)
    read = gc.read_gif(gif.assemble(units, w, h, palette))
    assert (read['width'], read['height'], read['loop'], read['packed']) == (w, h, 0, 0xF7) and np.array_equal(read['palette'][:len(palette)], palette)
    assert not read['palette'][len(palette):].any() and len(read['frames']) == 1
    frame = read['frames'][0]
    assert (frame['delay'], frame['disposal'], frame['transparent'], frame['left'], frame['top'], frame['width'], frame['height']) == (4, 0, 0, 0, 0, w, h)
    assert not frame['local_table'] and not frame['interlace'] and frame['min_code_size'] == 8
    assert np.array_equal(frame['indices'].reshape(h, w), table[gc.cells(frames[0], False, gc.DITHER)])
    segments = segments_of(frame['codes'])
    assert len(segments) == stats['segments'] == -(-h * w // gc.SEGMENT) and sum(len(s[0]) for s in segments) == stats['codes']
    assert sum(len(s[2]) for s in segments) == stats['pad_clears']
    widths = WIDTHS()
    block_ends, segment_ends = np.cumsum(frame['blocks']).tolist(), set()
    for i, (data, closing, pads) in enumerate(segments):
        start = data[0][2]
        assert all(width <= 12 for _, width, _ in data + [closing] + pads)
        for k, (value, width, position) in enumerate(data):
            assert (width, position - start) == widths[k], (i, k)
        assert closing[1] == widths[len(data)][0] and closing[2] - start == widths[len(data)][1]
        assert len(pads) <= 7 and all(p[1] == 9 for p in pads)
        end = (pads[-1] if pads else closing)
        end = end[2] + end[1]
        segment_ends.add(-(-end // 8))
        if i + 1 < len(segments):
            assert closing[0] == 256 and end % 8 == 0 and end // 8 in block_ends, 'a segment ends on a byte boundary, at the end of a sub-block'
        else:
            assert closing[0] == 257 and -(-end // 8) == sum(frame['blocks'])
    assert all(1 <= size <= 255 for size in frame['blocks']) and {end for size, end in zip(frame['blocks'], block_ends) if size < 255} <= segment_ends, 'a short sub-block is a segment\'s last'


def test_a_segment_holds_exactly_its_pixels(gif):
    """The decoded strings of a segment's codes add up to kSegmentPixels: cut where the Clears are, the indices are the frame's in raster order."""
    frames, (palette, table) = gc.case_frames('96x128', 1), gc.case_palette('96x128')
    units = gc.case_twin('96x128', 1)[0]
    codes = gc.read_gif(gif.assemble(units, 128, 96, palette))['frames'][0]['codes']
    # a fresh dictionary per segment: decode each segment's data codes on their own
    want = table[gc.cells(frames[0])].reshape(-1)
    for i, (data, _, _) in enumerate(segments_of(codes)):
        strings, previous = {}, None
        out = []
        for value, _, _ in data:
            string = (value,) if value < 256 else strings[value] if value in strings else previous + previous[:1]
            if previous is not None:
                strings[258 + len(strings)] = previous + string[:1]
            out.extend(string)
            previous = string
        assert np.array_equal(out, want[i * gc.SEGMENT:(i + 1) * gc.SEGMENT]), i


@pytest.mark.parametrize('name', sorted(set(gc.CASES) - {'widest', 'tallest'}) + ['widest'])
def test_the_kernels_steps_give_the_definitions_bytes(name):
    frames, table = gc.case_frames(name, 2), gc.case_palette(name, gc.BGR)[1]
    assert gc.twin(frames, table, gc.BGR, gc.DITHER, pieces=True)[0] == gc.twin(frames, table, gc.BGR, gc.DITHER)[0]


def test_the_bound(gif):
    units, _, segment, bound = gc.case_twin('no_pair_twice', 2)
    assert segment == gc.SEGMENT <= 3838
    assert [len(u) for u in units] == [bound, bound] == [gc.twin_bound(100, 90)] * 2             # every code covers one pixel: the unit is as long as the bound
    lib = gif.load()
    for w, h in [(1, 1), (100, 90), (101, 38), (349, 11), (65535, 2), (2, 65535), (1024, 1024), (30000, 20000)]:
        assert int(lib.kbe_gif_bound(w, h)) == gc.twin_bound(w, h) > 0, (w, h)
    for w, h in [(65535, 65535), (0, 5), (5, 0), (65536, 1), (1, 65536), (-1, 4), (40000, 40000)]:
        assert int(lib.kbe_gif_bound(w, h)) == 0, (w, h)
    # the closed form, restated: 19 + 1 bytes around the segments; a segment of n one-pixel codes takes [9 +] bits_before(n) + width(n) bits,
    # padded with Clears to a byte unless it is the last, in sub-blocks of 255
    def segment_bytes(n, first, last):
        width = lambda k: 9 + sum(258 + max(k - 1, 0) >= t for t in (512, 1024, 2048))
        bits = (9 if first else 0) + sum(width(k) for k in range(n)) + width(n)
        bits += 0 if last else 9 * (-bits % 8)
        data = -(-bits // 8)
        return data + -(-data // 255)
    pixels = 90 * 100
    full, rest = divmod(pixels, gc.SEGMENT)
    assert bound == 20 + segment_bytes(gc.SEGMENT, True, False) + (full - 1) * segment_bytes(gc.SEGMENT, False, False) + segment_bytes(rest, False, True)


# -- the palette ----------------------------------------------------------------------------
def test_few_colours_come_back_exactly(gif):
    rng = np.random.default_rng(11)
    cells = rng.choice(gc.CELLS, 256, replace=False)
    frame = gc.centres(cells)[rng.integers(0, 256, (40, 50))].astype(np.uint8)
    palette = gif.palette_from_histogram(gc.hist_of(frame))
    present = np.unique(gc.cells(frame))
    assert np.array_equal(palette, gc.centres(present))
    table = gc.lut_of(palette)
    units = gc.twin(frame[None], table)[0]
    assert np.array_equal(decoded(gif.assemble(units, 50, 40, palette))[1][0], frame)


def test_the_palette_is_deterministic_and_uses_all_its_entries(gif):
    hist = gc.hist_of(gc.case_frames('photo_like', 3))
    a, b = gif.palette_from_histogram(hist), gif.palette_from_histogram(hist.copy())
    assert a.dtype == np.uint8 and a.shape == (256, 3) and np.array_equal(a, b)
    assert gif.palette_from_histogram(hist, colors=16).shape == (16, 3)
    with pytest.raises(ValueError):
        gif.palette_from_histogram(np.zeros(gc.CELLS, np.int64))
    # counts as large as a long clip's: every count times 2^20 (6 * 10^10 pixels) moves no median, no mean and no order of the boxes' errors
    assert np.array_equal(gif.palette_from_histogram(hist << 20), a)


def test_the_palette_against_a_uniform_one_and_against_pillows_median_cut(gif):
    frames = gc.case_frames('photo_like', 3)
    palette = gif.palette_from_histogram(gc.hist_of(frames))
    ours = gc.psnr(palette[gc.lut_of(palette)[gc.cells(frames)]], frames)
    levels = lambda n: np.round(np.linspace(0, 255, n)).astype(np.int64)
    uniform = np.array([(r, g, b) for r in levels(6) for g in levels(7) for b in levels(6)], np.uint8)
    flat = gc.psnr(uniform[gc.lut_of(uniform)[gc.cells(frames)]], frames)
    pillow = gc.psnr(np.stack([np.asarray(Image.fromarray(f).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert('RGB')) for f in frames]), frames)
    print('PSNR: ours %.2f dB, uniform 6x7x6 %.2f dB, Pillow MEDIANCUT per frame %.2f dB' % (ours, flat, pillow))
    assert ours > flat                  # an adaptive palette that loses to a uniform one is broken
    # measured on these frames: ours 30.48 dB, Pillow's 31.17 dB (a palette per frame and 8 bits per channel against one palette for all
    # frames at 5 bits per channel), a shortfall of 0.69 dB; 0.5 dB on top for the spread from seed to seed (0.46 .. 0.82 dB over five more triples)
    assert ours > pillow - (0.69 + 0.5)


# -- the host side, the device calls replaced ---------------------------------------------------
def test_write_gif_forth_and_back_through_the_twin(gif, monkeypatch, tmp_path):
    frames = gc.case_frames('50x37', 3)
    seen = {}

    def encode(fr, lut, bgr=False, dither='ordered', delay_cs=4, cap=None):
        seen.update(bgr=bgr, dither=dither, delay_cs=delay_cs, calls=seen.get('calls', 0) + 1)
        return gc.twin(fr, lut, gc.BGR if bgr else 0, gif._amplitude(dither), delay_cs)[0]
    monkeypatch.setattr(gif, 'histogram', lambda fr, bgr=False: gc.hist_of(fr, bgr))
    monkeypatch.setattr(gif, 'lut', gc.lut_of)
    monkeypatch.setattr(gif, 'encode', encode)
    path = str(tmp_path / 'a.gif')
    palette, count = gif.write_gif(path, frames, fps=25, bgr=True)
    assert count == 5 and seen == dict(bgr=True, dither='ordered', delay_cs=4, calls=1)
    im, got = decoded(open(path, 'rb').read())
    assert im.n_frames == 5 and im.info['duration'] == 40 and im.info['loop'] == 0
    table = gc.lut_of(palette)
    for mine, i in zip(got, (0, 1, 2, 1, 0)):
        assert np.array_equal(mine, palette[table[gc.cells(frames[i], True, gc.DITHER)]])
    # every distinct frame once: the way back is the same units again
    units = gc.twin(frames, table, gc.BGR, gc.DITHER)[0]
    assert open(path, 'rb').read() == gif.assemble(units + units[-2::-1], 37, 50, palette)
    gif.write_gif(path, frames, fps=10, dither='none')
    assert seen['delay_cs'] == 10 and seen['dither'] == 'none' and decoded(open(path, 'rb').read())[0].info['duration'] == 100


def test_assemble(gif):
    palette = np.array([(1, 2, 3), (4, 5, 6)], np.uint8)
    data = gif.assemble([b'AB', b'C'], 300, 2, palette, loop=7)
    assert data[:13] == b'GIF89a' + bytes([44, 1, 2, 0, 0xF7, 0, 0]) and data[13:19] == bytes([1, 2, 3, 4, 5, 6]) and not any(data[19:13 + 768])
    assert data[13 + 768:] == b'\x21\xff\x0bNETSCAPE2.0\x03\x01\x07\x00\x00' + b'ABC' + b'\x3b'
    for bad in (dict(W=0), dict(W=65536), dict(loop=65536), dict(palette=np.zeros((257, 3), np.uint8)), dict(palette=np.zeros((0, 3), np.uint8))):
        with pytest.raises(ValueError):
            gif.assemble(**dict(dict(units=[b''], W=4, H=4, palette=palette), **bad))


def test_the_delay_rule(gif):
    assert [gif.delay_for(fps) for fps in (25, 24, 30, 50, 100, 10, 12.5, 1000)] == [4, 4, 3, 2, 2, 10, 8, 2]


def test_the_command_line():
    from ken_burns_effect_amd import kbe
    assert kbe.parse([])[0]['gif'] is False and kbe.parse([])[0]['gif-dither'] is None
    cfg = kbe.parse(['--gif', '--gif-dither', 'none'])[0]
    assert cfg['gif'] is True and cfg['gif-dither'] == 'none' and kbe.parse(['--gif'])[0]['gif-dither'] is None
    with pytest.raises(SystemExit):
        kbe.parse(['--gif', '--gif-dither', 'fast'])


def test_the_switches(monkeypatch):
    from ken_burns_effect_amd import pipeline as P
    monkeypatch.delenv('KBE_GIF', raising=False)
    monkeypatch.delenv('KBE_GIF_DITHER', raising=False)
    assert P.gif_switch() is False and P.gif_switch(True) is True and P.gif_dither() == 'ordered' and P.gif_dither('none') == 'none'
    monkeypatch.setenv('KBE_GIF', '1')
    monkeypatch.setenv('KBE_GIF_DITHER', 'none')
    assert P.gif_switch() is True and P.gif_switch(False) is False and P.gif_dither() == 'none'
    monkeypatch.setenv('KBE_GIF_DITHER', 'fast')
    with pytest.raises(ValueError):
        P.gif_dither()
