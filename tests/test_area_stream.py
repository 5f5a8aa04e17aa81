"""The exact area-average reduction (include/kbe_area.h) without a GPU: the NumPy twin's properties, csrc/kbe_area_block.h executed serially
(tests/area_check.cpp) against a brute-force restatement and against the twin, area.size_for, the command line's options, and the twin
beside Pillow's BOX filter."""
import re

import numpy as np
import pytest
from PIL import Image

import area_cases as ac
import gif_cases as gc


@pytest.mark.parametrize('N, n', [(160, 75), (128, 60), (160, 80), (160, 159), (160, 160), (128, 1), (17, 3), (16, 5), (1000, 333), (1000, 777), (65535, 3), (1, 1)])
def test_the_weights_add_up_to_the_cells_lengths(N, n):
    A = ac.weights(n, N)
    assert A.shape == (n, N) and A.dtype == np.int64 and A.min() >= 0 and A.max() <= n
    assert (A.sum(axis=1) == N).all() and (A.sum(axis=0) == n).all()
    # a target's sources are one run of cells, floor(o N / n) up to ceil((o + 1) N / n)
    o = np.arange(n, dtype=np.int64)
    first, last = (A != 0).argmax(axis=1), N - 1 - (A[:, ::-1] != 0).argmax(axis=1)
    assert np.array_equal(first, o * N // n) and np.array_equal(last + 1, -(-(o + 1) * N // n)) and np.array_equal((A != 0).sum(axis=1), last + 1 - first)


def test_a_constant_image_stays_constant():
    for value in (0, 1, 137, 254, 255):
        for (W, H), (w, h) in (((70, 50), (33, 21)), ((160, 128), (159, 127)), ((17, 16), (3, 5)), ((31, 33), (1, 1))):
            assert (ac.twin_reduce(np.full((H, W, 3), value, np.uint8), w, h) == value).all()


def test_integer_factors_are_the_box_mean_rounded_half_up():
    rng = np.random.default_rng(2)
    for (fx, fy), (w, h) in (((2, 2), (80, 64)), ((1, 3), (16, 7)), ((5, 1), (9, 11)), ((4, 7), (3, 2))):
        src = rng.integers(0, 256, (h * fy, w * fx, 3), dtype=np.uint8)
        total = src.reshape(h, fy, w, fx, 3).astype(np.int64).sum(axis=(1, 3))
        assert np.array_equal(ac.twin_reduce(src, w, h), (2 * total + fx * fy) // (2 * fx * fy))
    # half goes up: two pixels of 0 and 1 are 1, of 254 and 255 are 255
    assert ac.twin_reduce(np.array([[[0] * 3, [1] * 3]], np.uint8), 1, 1).tolist() == [[[1, 1, 1]]]
    assert ac.twin_reduce(np.array([[[254] * 3], [[255] * 3]], np.uint8), 1, 1).tolist() == [[[255, 255, 255]]]


def test_the_same_size_is_the_identity():
    frames = ac.photo(2)
    assert np.array_equal(ac.twin_reduce(frames, 160, 128), frames)
    assert np.array_equal(ac.twin_reduce(ac.small(), 17, 16), ac.small())


def test_the_header_against_brute_force():
    """area_check.cpp builds, and csrc/kbe_area_block.h run serially equals the restatement on sub-cells at every size up to 6 x 6."""
    m = re.search(r'brute: cases (\d+), pixels (\d+), mismatches (\d+), bad sums (\d+), bad spans (\d+), bad windows (\d+)', ac.ask('brute', 6))
    cases, pixels, mismatches, bad_sums, bad_spans, bad_windows = (int(v) for v in m.groups())
    assert cases == 3 * 21 * 21 and pixels == 3 * 56 * 56 and mismatches == 0 and bad_sums == 0 and bad_spans == 0 and bad_windows == 0
    m = re.search(r'limits: weights (\d+), bad (\d+)', ac.ask('limits'))
    assert int(m.group(1)) > 50 and int(m.group(2)) == 0


@pytest.mark.parametrize('name', sorted(ac.TARGETS))
def test_the_header_is_the_twin(name):
    """reduce_pixel of csrc/kbe_area_block.h on the GPU suite's frames, rows padded: the NumPy twin byte for byte."""
    w, h = ac.TARGETS[name]
    assert np.array_equal(ac.header_reduce(ac.photo(2), w, h, pad=5), ac.twin_of(name, 2))


def test_the_header_is_the_twin_below_a_tile():
    assert np.array_equal(ac.header_reduce(ac.small(), 3, 5), ac.twin_reduce(ac.small(), 3, 5))


def test_size_for():
    from ken_burns_effect_amd import area
    for W, H in ((1024, 1024), (1024, 768), (160, 128), (17, 16), (65535, 3), (3, 65535)):
        assert area.size_for(W, H) == (W, H) == area.size_for(W, H, width=W) == area.size_for(W, H, height=H)
        for side in (1, 2, 3, 7, 64, 480, 1000):
            if side <= W:
                assert area.size_for(W, H, width=side) == (side, max(1, (H * side + W // 2) // W))
            if side <= H:
                assert area.size_for(W, H, height=side) == (max(1, (W * side + H // 2) // H), side)
            if side <= W and side <= H:
                assert area.size_for(W, H, width=side, height=side) == (side, side)
    assert area.size_for(1024, 1024, width=480) == (480, 480) and area.size_for(1024, 768, width=480) == (480, 360) and area.size_for(128, 96, width=64) == (64, 48)
    assert area.size_for(65535, 3, width=1) == (1, 1) and area.size_for(3, 2, width=2) == (2, 1) and area.size_for(3, 2, height=1) == (2, 1)      # (halves go up)
    for bad in (dict(width=161), dict(height=129), dict(width=0), dict(height=-1), dict(width=160, height=129)):
        with pytest.raises(ValueError, match='only reduced'):
            area.size_for(160, 128, **bad)
    with pytest.raises(ValueError):
        area.size_for(65536, 16, width=4)


def test_kept_frames_and_the_delay():
    from ken_burns_effect_amd import gif
    assert gif.kept_frames(75, 1) == list(range(75))
    assert gif.kept_frames(75, 2) == list(range(0, 75, 2))                    # (74 is the last frame)
    assert gif.kept_frames(75, 3) == list(range(0, 75, 3)) + [74]
    assert gif.kept_frames(2, 2) == [0, 1] and gif.kept_frames(1, 5) == [0] and gif.kept_frames(13, 100) == [0, 12]
    with pytest.raises(ValueError):
        gif.kept_frames(5, 0)
    assert gif.delay_for(25 / 2.0) == 8 and gif.delay_for(25) == 4


def test_the_command_line_takes_and_refuses_the_gif_options(tmp_path, monkeypatch):
    from ken_burns_effect_amd import kbe, pipeline
    cfg, _ = kbe.parse(['--gif', '--gif-width', '480', '--gif-fps', '12.5'])
    assert cfg['gif'] is True and cfg['gif-width'] == 480 and cfg['gif-fps'] == 12.5
    cfg, _ = kbe.parse(['--gif'])
    assert cfg['gif-width'] is None and cfg['gif-fps'] is None
    for argv, text in ((['--gif-width', '480'], 'only with --gif'), (['--gif-fps', '10'], 'only with --gif'), (['--gif', '--gif-width', '0'], '1 or more'),
                       (['--gif', '--gif-width', '4.5'], '1 or more'), (['--gif', '--gif-fps', '0'], 'above 0'), (['--gif', '--gif-fps', 'fast'], 'above 0')):
        with pytest.raises(SystemExit, match=text):
            kbe.parse(argv)
    # every = max(1, round(25 / F))
    monkeypatch.delenv('KBE_GIF_WIDTH', raising=False)
    monkeypatch.delenv('KBE_GIF_FPS', raising=False)
    assert pipeline.gif_shape() == (None, 1)
    for fps, every in ((25, 1), (100, 1), (12.5, 2), (12, 2), (8, 3), (5, 5), (1, 25), (15, 2)):
        assert pipeline.gif_shape(None, fps) == (None, every) == (None, max(1, round(25 / fps)))
    monkeypatch.setenv('KBE_GIF_WIDTH', '64')
    monkeypatch.setenv('KBE_GIF_FPS', '12.5')
    assert pipeline.gif_shape() == (64, 2) and pipeline.gif_shape(32, 25) == (32, 1)
    monkeypatch.setenv('KBE_GIF_WIDTH', 'wide')
    with pytest.raises(ValueError, match='KBE_GIF_WIDTH'):
        pipeline.gif_shape()
    # a width above the image's: a plain message, before any network is built
    monkeypatch.delenv('KBE_GIF_WIDTH')
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(32, 48, 1)).save(path)
    import torch
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        with pytest.raises(SystemExit, match='--gif-width 49: the image is 48 pixels wide'):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--gif', '--gif-width', '49'])
    finally:
        torch.set_grad_enabled(grad)


# the largest difference per byte between the twin and Pillow's BOX filter, measured (Pillow 12.2) on 160 x 128 sources: {target: (photo_like, noise)}
PILLOW_MEASURED = {(1, 1): (0, 0), (80, 64): (1, 1), (40, 32): (1, 1), (32, 16): (1, 1), (160, 128): (0, 0),
                   (75, 60): (27, 57), (159, 127): (60, 156), (53, 128): (19, 39), (160, 41): (15, 36)}


def test_the_twin_beside_pillows_box_filter():
    """The twin beside Pillow's resize(..., Image.BOX), a cross-check and not the definition.

    Where every target covers whole source pixels (integer factors, the copy, one pixel) Pillow's filter is the same average taken in two
    passes with a rounding to 8 bits between them, and the two differ by at most 1 count per byte: measured 38 % of the bytes at a factor
    of 2 (photo_like and noise alike), 22 % at 4, 8-10 % at 5 x 8, none for the copy and for one pixel.

    At any other ratio Pillow's BOX filter is no area average: it counts a source pixel wholly or not at all, by where its centre falls,
    where this project weighs it by the overlap.  There the difference is far above 1 -- measured: photo_like -> 75x60 up to 27 counts
    (61 % of the bytes differ), -> 159x127 up to 60 (78 %), noise -> 75x60 up to 57 (97 %), -> 159x127 up to 156 (99 %) -- so for those
    targets this check only holds the measured maximum plus 1 (PILLOW_MEASURED).  The twin stays the definition: tests/area_check.cpp holds
    it to the restatement on sub-cells, which is the area average by construction."""
    cases = [('photo_like', ac.photo(1)[0]), ('noise', gc.noise(128, 160, 5))]
    for kind, (name, src) in enumerate(cases):
        for (w, h), measured in sorted(PILLOW_MEASURED.items()):
            ours = ac.twin_reduce(src, w, h).astype(np.int64)
            theirs = np.asarray(Image.fromarray(src).resize((w, h), Image.BOX)).astype(np.int64)
            diff = np.abs(ours - theirs)
            print('%s 160x128 -> %dx%d: max %d, differing %.4f' % (name, w, h, diff.max(), (diff > 0).mean()))
            whole_pixels = 160 % w == 0 and 128 % h == 0
            assert diff.max() <= (1 if whole_pixels else measured[kind] + 1), (name, w, h)
