"""The colour grade (include/kbe_grade.h) without a GPU: csrc/kbe_grade_block.h executed serially (tests/grade_check.cpp) against the plain
definition on all 2^24 colours and against the NumPy twin (tests/grade_cases.py) on the GPU suite's cases; the twin against the float64
reference; every refusal of the entry on host memory; read_cube on files written here, a good one and every refusal; bake, compose,
resample and quantise on values that can be stated by hand; and the options of the two command lines and of Pipeline, with every refusal
raised before a network is built."""
import ctypes
import os
import re
import warnings
from ctypes import c_int32, c_void_p

import numpy as np
import pytest
from PIL import Image

import gif_cases
import grade_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 17, 33])
def test_the_packed_forms_are_the_plain_ones_on_every_colour(N):
    """grade_check.cpp builds; all 2^24 colours through a random table of N nodes per axis: the packed form against the plain one, every
    tie between fractions at all six orders of the axes, the float interpolation of the same nodes within 0.5.  All mismatch counts are zero."""
    m = re.search(r'brute: N (\d+), colours (\d+), packed mismatches (\d+), ties (\d+), tie mismatches (\d+), float mismatches (\d+), range mismatches (\d+)', gc.ask('brute', N))
    size, colours, packed, ties, tie_bad, float_bad, range_bad = (int(v) for v in m.groups())
    assert size == N and colours == 1 << 24 and ties >= 3 * 256 * 256 - 2 * 256
    assert (packed, tie_bad, float_bad, range_bad) == (0,) * 4


def test_the_cells_the_divisions_the_mix_and_the_rows():
    """Every (N, byte): the cell and fraction without a divide against / 255; all 256 x 256 x 257 (c, g, s) of the strength's mix in every
    lane; the run's packing and realignment against the bytes; whole rows at all four classes and twelve widths against the plain form."""
    m = re.search(r'forms: cells (\d+), cell mismatches (\d+), mixes (\d+), mix mismatches (\d+), run mismatches (\d+), rows (\d+), row mismatches (\d+)', gc.ask('forms'))
    cells, cell_bad, mixes, mix_bad, run_bad, rows, row_bad = (int(v) for v in m.groups())
    assert cells == 32 * 256 and mixes == 256 * 256 * 257 and rows == 12 * 4 * 8
    assert (cell_bad, mix_bad, run_bad, row_bad) == (0,) * 4


def test_the_identity_table_is_exact_where_its_nodes_are_and_within_one_everywhere():
    m = re.search(r'identity: lattice (\d+), beyond one (\d+), exact sizes (\d+), inexact on the lattice (\d+), all colours (\d+), inexact (\d+)', gc.ask('identity'))
    lattice, beyond, exact_sizes, inexact, full, full_bad = (int(v) for v in m.groups())
    assert lattice == 32 * 3 * 256 * 24 * 24 and exact_sizes == 5 == len(gc.EXACT_SIZES) and full == 5 << 24
    assert [N for N in range(2, 34) if 255 % (N - 1) == 0] == list(gc.EXACT_SIZES)
    assert (beyond, inexact, full_bad) == (0,) * 3


def test_the_pinned_values():
    """Values stated by hand, for the twin and for the header through flat frames."""
    assert [tuple(int(v) for v in gc.cells(v, N)) for v, N in ((0, 2), (254, 2), (255, 2), (16, 17), (15, 17), (255, 17), (128, 33), (255, 33))] == \
        [(0, 0), (0, 254), (0, 255), (1, 1), (0, 240), (15, 255), (16, 16), (31, 255)]
    # N = 2, the corners black but the far one white: a grey v has three equal fractions, so g = (255 v + 127) / 255 = v on the diagonal
    corner = np.zeros((2, 2, 2, 4), np.uint8)
    corner[1, 1, 1, :3] = 255
    for grade in (gc.twin_grade, gc.header_grade):
        flat = np.full((1, 2, 5, 3), 100, np.uint8)
        assert (grade(flat, corner, 256) == 100).all() and (grade(flat, corner, 128) == 100).all()
        # (200, 100, 50): f = (200, 100, 50), weights 55, 100, 50, 50: only the far corner is white -> (255 * 50 + 127) / 255 = 50
        pixel = np.tile(np.asarray([200, 100, 50], np.uint8), (1, 3, 4, 1))
        assert (grade(pixel, corner, 256) == 50).all()
        # at strength 128: (c * 128 + 50 * 128 + 128) >> 8 = (125, 75, 50)
        assert (grade(pixel, corner, 128) == (125, 75, 50)).all()
        assert np.array_equal(grade(pixel, corner, 0), pixel)
        # the axes: a table whose node at byte 0's far end alone is white answers byte 0
        axis = np.zeros((2, 2, 2, 4), np.uint8)
        axis[0, 0, 1, :3] = 255                                            # [i2, i1, i0]
        assert (grade(pixel, axis, 256) == (200 - 100) * 255 // 255).all() and (grade(pixel[..., ::-1].copy(), axis, 256) == 0).all()


@pytest.mark.parametrize('kind', ['random', 'rotation'])
@pytest.mark.parametrize('N', gc.SIZES)
@pytest.mark.parametrize('frame', gc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_header_is_the_twin(frame, N, kind):
    """grade_row of csrc/kbe_grade_block.h on the GPU suite's cases, the rows padded by 5 (every row at another alignment): the NumPy twin byte for byte."""
    W, H = frame
    want = gc.twin_of(W, H, N, kind)
    assert np.array_equal(gc.header_grade(gc.frames_of(W, H), gc.TABLES[kind](N), gc.STRENGTH, pad=5), want)
    assert (want != gc.frames_of(W, H)).any(axis=3).mean() > 0.5


def test_the_header_on_the_other_cases():
    """All 64^3 combinations of the cells' edges; a constant table; exact identities; a baked sepia; W = 1 and rows of 4098 bytes; strength 0."""
    frame = gc.all_cells_frame()
    for N in (17, 33):
        assert np.array_equal(gc.header_grade(frame, gc.random(N), 256), gc.twin_grade(frame, gc.random(N), 256))
    frames = gc.frames_of(37, 12, 3)
    assert (gc.header_grade(frames, gc.constant(33), 256, pad=1) == (17, 200, 99)).all()
    for N in gc.EXACT_SIZES:
        assert np.array_equal(gc.header_grade(frames, gc.identity(N), 256, pad=3), frames) and np.array_equal(gc.twin_grade(frames, gc.identity(N), 256), frames)
    assert np.array_equal(gc.header_grade(frames, gc.sepia(), (256, 192, 1), pad=2), gc.twin_grade(frames, gc.sepia(), (256, 192, 1)))
    assert np.array_equal(gc.header_grade(frames, gc.random(5), (0, 77, 0)), gc.twin_grade(frames, gc.random(5), (0, 77, 0)))
    assert np.array_equal(gc.twin_grade(frames, gc.random(5), (0, 77, 0))[[0, 2]], frames[[0, 2]])
    for W, H in ((1, 7), (1366, 3)):
        odd = gc.frames_of(W, H)
        assert np.array_equal(gc.header_grade(odd, gc.random(33), (256, 77), pad=1), gc.twin_grade(odd, gc.random(33), (256, 77)))


@pytest.mark.parametrize('N', [2, 3, 17, 25, 33])
def test_the_twin_is_within_one_of_the_float_reference(N):
    """Derived, not measured: g is the nearest whole number to the exact combination of the table's nodes, so it lies within 0.5 of the float
    interpolation of the same nodes; against nodes that were rounded from unrounded ones (at most 0.5 each, which a convex combination
    keeps) that is 1."""
    frames = np.concatenate([gc.frames_of(160, 128), gc.all_cells_frame()[:, :128, :160]])
    table = gc.random(N)
    got = gc.twin_grade(frames, table, 256).astype(np.float64)
    assert np.abs(got - gc.float_grade(frames, table)).max() <= 0.5 + 1e-9
    # ... and with unrounded nodes: a float table, quantised for the twin, against grade.interpolate on the float table
    from ken_burns_effect_amd import grade
    smooth = grade.bake(contrast=1.3, saturation=0.6, gamma=1.7, N=N)
    device = np.ascontiguousarray(grade.quantise(smooth, False)).view(np.uint8).reshape(N, N, N, 4)
    exact = 255.0 * grade.interpolate(smooth, frames.astype(np.float64) / 255.0)
    assert np.abs(gc.twin_grade(frames, device, 256) - exact).max() <= 1.0 + 1e-9


# -- the entry's refusals on host memory ---------------------------------------------------------
# (frames of 16 x 17 at a stride of 48: 816 bytes, at 0 and 2048 of 64 KiB of host memory; the table, 5^3 dwords: 500 bytes, at 8192)
OVERLAPS_FRAME, OVERLAPS_TABLE = 'an element of frames_u8 overlaps another frame', 'an element of frames_u8 overlaps the table'
REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null lut': (dict(lut=None), 'null lut'), 'null strength': (dict(strength=None), 'null strength'),
           'n = 0': (dict(n=0), 'n < 1'), 'n = -1': (dict(n=-1), 'n < 1'), 'W = 0': (dict(W=0), 'W or H outside 1..65535'),
           'W = 65536': (dict(W=65536, stride_bytes=3 * 65536), 'W or H outside 1..65535'), 'H = 0': (dict(H=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'),
           'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'), 'N = 1': (dict(N=1), 'N outside 2..33'), 'N = 34': (dict(N=34), 'N outside 2..33'), 'N = 0': (dict(N=0), 'N outside 2..33'),
           'a table one byte off': (dict(lut=8193), 'lut is not 4-byte aligned'), 'a table two bytes off': (dict(lut=8194), 'lut is not 4-byte aligned'),
           'null frame 1': (dict(frames_u8=(None, 0)), 'null element of frames_u8'),
           'strength 257': (dict(strength=(256, 257)), 'an element of strength outside 0..256'), 'strength -1': (dict(strength=(-1, 256)), 'an element of strength outside 0..256'),
           'the same frame twice': (dict(frames_u8=(None, 1)), OVERLAPS_FRAME), 'one byte into the next frame': (dict(frames_u8=(2048 - 815 + 1, None)), OVERLAPS_FRAME),
           'the table is a frame': (dict(lut=2048), OVERLAPS_TABLE), 'the table on a frames last dword': (dict(lut=812), OVERLAPS_TABLE),
           'a frame on the tables last byte': (dict(frames_u8=(None, 8192 + 499 + 1)), OVERLAPS_TABLE),
           # (at strength 0 nothing would be launched, and the overlap is refused all the same)
           'an overlap of frames that are in no launch': (dict(frames_u8=(None, 1), strength=(0, 0)), OVERLAPS_FRAME)}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, grade
    memory = (ctypes.c_uint64 * 8192)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 2)(at, at + 2048), n=2, W=16, H=17, stride_bytes=48, lut=at + 8192, N=5, strength=(c_int32 * 2)(256, 128), stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key == 'frames_u8' and isinstance(value, tuple):
            for k in (0, 1):                                                # (None: as it was; 0: null; 1: the other frame's pointer; else an offset)
                if value[k] is not None:
                    args[key][k] = None if value[k] == 0 else args[key][1 - k] if value[k] == 1 else at + value[k] - 1
        elif key == 'strength' and value is not None:
            args[key] = (c_int32 * 2)(*value)
        elif key == 'lut' and value is not None:
            args[key] = at + value
        else:
            args[key] = value
    assert grade._raw('kbe_grade_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_grade_u8: ' + text
    assert not any(memory)


def test_apply_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, grade
    good, table = torch.zeros(4, 8, 8, 3, dtype=torch.uint8), torch.zeros(5, 5, 5, 4, dtype=torch.uint8)
    for bad in (good, np.zeros((4, 8, 8, 3), np.uint8), torch.zeros(4, 8, 8, 3), torch.zeros(8, 8, 3, dtype=torch.uint8), None):
        with pytest.raises(_native.KbeError, match=r'grade\.apply'):
            grade.apply(bad, table)


# -- .cube files -------------------------------------------------------------------------------
def _cube(path, N, rows=None, head=None, tail=''):
    """A .cube file of the table T[r, g, b] = (r / (N - 1), g / (N - 1) / 2, 1 - b / (N - 1)), red fastest, or of `rows` as they are."""
    lines = ['# a comment', 'TITLE "a test, with LUT_3D_SIZE in it"', '', 'LUT_3D_SIZE %d' % N, 'DOMAIN_MIN 0.0 0.0 0.0', 'DOMAIN_MAX 1.0 1 1.0'] if head is None else list(head)
    if rows is None:
        rows = ['%.6f %.6f %.6f' % (r / (N - 1), g / (N - 1) / 2, 1 - b / (N - 1)) for b in range(N) for g in range(N) for r in range(N)]
    with open(path, 'w') as f:
        f.write('\n'.join(lines + ['  # the rows', ''] + list(rows)) + '\n' + tail)
    return str(path)


def test_read_cube_reads_a_good_file(tmp_path):
    from ken_burns_effect_amd import grade
    for N in (2, 5, 33):
        t = grade.read_cube(_cube(tmp_path / ('good%d.cube' % N), N))
        assert t.shape == (N, N, N, 3) and t.dtype == np.float64 and t.flags['C_CONTIGUOUS']
        r, g, b = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing='ij')
        assert np.abs(t - np.stack([r / (N - 1), g / (N - 1) / 2, 1 - b / (N - 1)], axis=-1)).max() < 1e-6
    # no domain lines, no title, exponents and a row of whole numbers
    path = _cube(tmp_path / 'bare.cube', 2, rows=['0 0 0', '1 0 0', '0 1e0 0', '1 1 0', '0 0 1', '1 0 1', '0 1 1', '1 1 1.5'], head=['LUT_3D_SIZE 2'])
    t = grade.read_cube(path)
    assert np.array_equal(t[..., :2], grade.grid(2)[..., :2]) and t[1, 1, 1, 2] == 1.5 and t[1, 0, 0].tolist() == [1, 0, 0] and t[0, 0, 1].tolist() == [0, 0, 1]


def test_read_cube_refuses_with_the_file_and_the_line(tmp_path):
    from ken_burns_effect_amd import grade
    eight = ['0 0 0'] * 8
    cases = (
        (dict(N=2, head=['LUT_1D_SIZE 2'], rows=['0 0 0', '1 1 1']), 1, r'LUT_1D_SIZE: a 1D table'),
        (dict(N=2, head=['TITLE "x"', 'LUT_3D_SIZE 2', 'DOMAIN_MIN 0 0 0', 'DOMAIN_MAX 2 2 2'], rows=eight), 4, r'DOMAIN_MAX 2 2 2: only the domain 0 0 0 \.\. 1 1 1'),
        (dict(N=2, head=['LUT_3D_SIZE 2', 'DOMAIN_MIN -1 0 0'], rows=eight), 2, r'DOMAIN_MIN -1 0 0: only the domain'),
        (dict(N=2, head=['LUT_3D_SIZE 1'], rows=['0 0 0']), 1, r'LUT_3D_SIZE 1: a whole number 2\.\.256'),
        (dict(N=2, head=['LUT_3D_SIZE 257'], rows=eight), 1, r'LUT_3D_SIZE 257: a whole number 2\.\.256'),
        (dict(N=2, head=['LUT_3D_SIZE two'], rows=eight), 1, r'LUT_3D_SIZE two: a whole number'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:7]), 10, r'7 rows for LUT_3D_SIZE 2: 8 are needed'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight + ['1 1 1']), 12, r'more than the 8 rows of LUT_3D_SIZE 2'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:3] + ['0 0'] + eight[:4]), 7, r"a malformed row '0 0': three numbers"),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:3] + ['0 0 0 0'] + eight[:4]), 7, r'a malformed row'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:3] + ['0 0.5x 0'] + eight[:4]), 7, r'a malformed row'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:2] + ['0 nan 0'] + eight[:5]), 6, r'a number that is not finite'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:2] + ['inf 0 0'] + eight[:5]), 6, r'a number that is not finite'),
        (dict(N=2, head=['LUT_3D_SIZE 2'], rows=eight[:2] + ['0 0 -1e999'] + eight[:5]), 6, r'a number that is not finite'),
        (dict(N=2, head=[], rows=eight), 3, r'a row of numbers before LUT_3D_SIZE'),
        (dict(N=2, head=['LUT_3D_SIZE 2', 'LUT_3D_SIZE 2'], rows=eight), 2, r'LUT_3D_SIZE twice'),
        (dict(N=2, head=['LUT_3D_SIZE 2', 'LUT_SHAPER 4'], rows=eight), 2, r'unknown keyword LUT_SHAPER'),
        (dict(N=2, head=['TITLE "nothing else"'], rows=[]), 1, r'no LUT_3D_SIZE'))
    for k, (kw, line, text) in enumerate(cases):
        path = _cube(tmp_path / ('bad%d.cube' % k), **kw)
        with pytest.raises(ValueError, match=r'^%s: line %d: %s' % (re.escape(path), line, text)):
            grade.read_cube(path)
    with pytest.raises(OSError):
        grade.read_cube(str(tmp_path / 'none.cube'))


# -- tables by hand ----------------------------------------------------------------------------
def test_bake_against_hand_written_values():
    from ken_burns_effect_amd import grade
    assert np.array_equal(grade.bake(), grade.grid(33)) and np.array_equal(grade.bake(saturation=1, N=5), grade.grid(5)) and grade.bake(N=2).shape == (2, 2, 2, 3)
    assert grade.grid(3)[2, 1, 0].tolist() == [1.0, 0.5, 0.0]
    mono = grade.bake(look='mono', N=9)
    assert np.ptp(mono, axis=-1).max() == 0.0 and np.allclose(mono[..., 0], (grade.grid(9) * grade.LUMA).sum(axis=-1)) and np.array_equal(mono, grade.bake(look='mono', saturation=3, N=9))
    assert np.allclose(grade.bake(saturation=0, N=9), mono) and grade.LUMA == (0.299, 0.587, 0.114)
    sepia = grade.bake(look='sepia', N=9)
    assert np.allclose(sepia, np.clip(mono[..., :1] * np.asarray(grade.SEPIA_TINT), 0, 1)) and sepia[0, 0, 0].tolist() == [0, 0, 0] and np.allclose(sepia[8, 8, 8], grade.SEPIA_TINT)
    # one node through every step: (0.5, 0.25, 1.0) at brightness 0.8 -> (0.4, 0.2, 0.8); contrast 1.5 -> (0.35, 0.05, 0.95);
    # Y = 0.299 * 0.35 + 0.587 * 0.05 + 0.114 * 0.95 = 0.2423; saturation 2 -> (0.4577, -0.1423, 1.6577); clamp -> (0.4577, 0, 1); gamma 2 -> sqrt
    t = grade.bake(brightness=0.8, contrast=1.5, saturation=2, gamma=2, N=5)
    assert np.allclose(t[2, 1, 4], [0.4577 ** 0.5, 0.0, 1.0], atol=1e-12)
    assert np.allclose(grade.bake(brightness=2, N=3)[1, 2, 0], [1.0, 1.0, 0.0]) and np.allclose(grade.bake(contrast=0, N=3), 0.5) and np.allclose(grade.bake(gamma=0.5, N=3)[1, 1, 1], 0.25)
    for kw in (dict(brightness=-0.1), dict(brightness=4.1), dict(contrast=5), dict(saturation=-1), dict(gamma=0.05), dict(gamma=11), dict(gamma=float('nan')), dict(brightness='1'),
               dict(look='teal'), dict(N=1), dict(N=2.5)):
        with pytest.raises(ValueError, match=r'^grade\.bake: '):
            grade.bake(**kw)


def test_compose_resample_and_interpolate_against_hand_written_values():
    from ken_burns_effect_amd import grade
    # N = 2, the corners black but the far one white: the value is the least of the three channels
    corner = np.zeros((2, 2, 2, 3))
    corner[1, 1, 1] = 1.0
    assert np.allclose(grade.interpolate(corner, [[0.8, 0.4, 0.2], [0.1, 0.9, 0.5], [1, 1, 1], [2, -1, 0.5]]), [[0.2] * 3, [0.1] * 3, [1] * 3, [0] * 3])
    # the axes: T[r, g, b]
    red = np.zeros((2, 2, 2, 3))
    red[1, 0, 0] = (1.0, 0.5, 0.25)
    assert np.allclose(grade.interpolate(red, [0.8, 0.4, 0.2]), np.asarray([1.0, 0.5, 0.25]) * 0.4) and np.allclose(grade.interpolate(red, [0.2, 0.4, 0.8]), 0.0)
    for N, M in ((2, 9), (5, 9), (9, 5), (33, 17), (64, 33)):
        assert np.abs(grade.resample(grade.grid(N), M) - grade.grid(M)).max() < 1e-12
    sepia = grade.bake(look='sepia', N=9)
    assert np.allclose(grade.compose(sepia, grade.grid(4)), sepia) and np.allclose(grade.compose(grade.grid(9), sepia), sepia) and grade.compose(grade.grid(5), sepia).shape == (5, 5, 5, 3)
    # first, then: brightness 0.5 followed by a table that swaps red and blue
    swap = grade.grid(3)[..., ::-1].copy()
    assert np.allclose(grade.compose(grade.bake(brightness=0.5, N=5), swap)[4, 2, 0], [0.0, 0.25, 0.5])
    # a node outside [0, 1] is clamped on its way into the next table
    assert np.allclose(grade.compose(grade.grid(3) * 2.0 - 0.5, grade.grid(2))[2, 0, 1], [1.0, 0.0, 0.5])
    for bad in (np.zeros((2, 2, 3)), np.zeros((2, 3, 2, 3)), np.zeros((1, 1, 1, 3)), np.full((2, 2, 2, 3), np.nan)):
        with pytest.raises(ValueError):
            grade.resample(bad, 3)


def test_quantise_against_hand_written_values():
    from ken_burns_effect_amd import grade
    t = grade.grid(3) * [1.0, 0.5, 0.25]                                     # T[r, g, b] = (r / 2, g / 4, b / 8)
    rgb, bgr = grade.quantise(t, False), grade.quantise(t, True)
    assert rgb.dtype == bgr.dtype == np.uint32 and rgb.shape == bgr.shape == (3, 3, 3) and rgb.flags['C_CONTIGUOUS'] and bgr.flags['C_CONTIGUOUS']
    # R, G, B frames: entry [i2 = b, i1 = g, i0 = r], bytes R, G, B
    assert rgb[2, 1, 0] == 0 | (64 << 8) | (64 << 16) and rgb[0, 0, 2] == 255 and rgb[0, 2, 1] == 128 | (128 << 8)
    # B, G, R frames: entry [i2 = r, i1 = g, i0 = b], bytes B, G, R
    assert bgr[2, 1, 0] == 0 | (64 << 8) | (255 << 16) and bgr[0, 0, 2] == 64 and bgr[1, 2, 0] == (128 << 8) | (128 << 16)
    # a BGR table is the RGB one transposed, its bytes in the other order
    a, b = rgb.view(np.uint8).reshape(3, 3, 3, 4), bgr.view(np.uint8).reshape(3, 3, 3, 4)
    assert np.array_equal(b[..., :3], a.transpose(2, 1, 0, 3)[..., 2::-1]) and (a[..., 3] == 0).all() and (b[..., 3] == 0).all()
    # clamped, round(255 x)
    assert grade.quantise(np.full((2, 2, 2, 3), 1.7), True)[0, 0, 0] == 0xFFFFFF and grade.quantise(np.full((2, 2, 2, 3), -0.2), True)[1, 1, 1] == 0
    assert grade.quantise(np.full((2, 2, 2, 3), 0.5), True)[0, 0, 0] == 0x808080 and grade.quantise(np.full((2, 2, 2, 3), 0.4999 / 255), False)[0, 0, 0] == 0
    # the identity, quantised, is the cases' identity table; a channel-asymmetric frame tells the two orders apart
    for N in (2, 16, 17, 33):
        assert np.array_equal(grade.quantise(grade.grid(N), True).view(np.uint8).reshape(N, N, N, 4)[..., :3], gc.identity(N)[..., :3])
    frames = gc.frames_of(37, 12, 1)
    warm = grade.bake(look='sepia', N=17)
    as_bgr = gc.twin_grade(frames, grade.quantise(warm, True).view(np.uint8).reshape(17, 17, 17, 4))
    as_rgb = gc.twin_grade(frames[..., ::-1].copy(), grade.quantise(warm, False).view(np.uint8).reshape(17, 17, 17, 4))
    assert np.array_equal(as_bgr, as_rgb[..., ::-1]) and (as_bgr[..., 2].astype(int) >= as_bgr[..., 0]).all() and (as_bgr[..., 2] > as_bgr[..., 0]).any()      # (B, G, R: red over blue)
    with pytest.raises(ValueError, match=r'^grade\.quantise: a table of 34 nodes per axis: 2\.\.33'):
        grade.quantise(grade.grid(34), True)


# -- the command lines -------------------------------------------------------------------------
ENV = ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_JPEG', 'KBE_PNG', 'KBE_OVERLAY', 'KBE_OVERLAY_AT', 'KBE_OVERLAY_OPACITY', 'KBE_CAPTION', 'KBE_CAPTION_AT', 'KBE_CAPTION_SIZE',
       'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES', 'KBE_Y4M', 'KBE_LUT', 'KBE_GRADE', 'KBE_LOOK', 'KBE_LUT_STRENGTH')
KEYS = 'brightness, contrast, saturation, gamma'


def _files(tmp_path):
    paths = {'good': _cube(tmp_path / 'look.cube', 4), 'big': _cube(tmp_path / 'big.cube', 35), 'none': str(tmp_path / 'none.cube'),
             'short': _cube(tmp_path / 'short.cube', 2, rows=['0 0 0'] * 7, head=['LUT_3D_SIZE 2']), 'one': _cube(tmp_path / 'one.cube', 2, rows=['0 0 0', '1 1 1'], head=['LUT_1D_SIZE 2'])}
    paths['text'] = str(tmp_path / 'notes.cube')
    with open(paths['text'], 'w') as f:
        f.write('not a table\n')
    return paths


def _refusals(P):
    return (
        (['--lut', P['none']], r'^--lut %s: no such file$' % re.escape(P['none'])), (['--lut', P['text']], r'^--lut %s: line 1: unknown keyword not$' % re.escape(P['text'])),
        (['--lut', P['short']], r'^--lut %s: line \d+: 7 rows for LUT_3D_SIZE 2: 8 are needed$' % re.escape(P['short'])),
        (['--lut', P['one']], r'^--lut %s: line 1: LUT_1D_SIZE: a 1D table; only 3D tables are taken$' % re.escape(P['one'])),
        (['--grade', 'hue=1'], r'^--grade hue=1: unknown key hue: %s$' % KEYS), (['--grade', 'contrast'], r'^--grade contrast: contrast=None: 0\.\.4$'),
        (['--grade', 'contrast=4.5'], r'^--grade contrast=4\.5: contrast=4\.5: 0\.\.4$'), (['--grade', 'brightness=-1'], r'^--grade brightness=-1: brightness=-1: 0\.\.4$'),
        (['--grade', 'gamma=0'], r'^--grade gamma=0: gamma=0: 0\.1\.\.10$'), (['--grade', 'gamma=11,contrast=1'], r'^--grade gamma=11,contrast=1: gamma=11: 0\.1\.\.10$'),
        (['--grade', 'saturation=lots'], r'^--grade saturation=lots: saturation=lots: 0\.\.4$'), (['--grade', 'saturation=nan'], r'^--grade saturation=nan: saturation=nan: 0\.\.4$'),
        (['--grade', 'contrast=1,contrast=2'], r'^--grade contrast=1,contrast=2: contrast twice$'), (['--grade', 'contrast=1,,gamma=2'], r'^--grade contrast=1,,gamma=2: unknown key : '),
        (['--look', 'teal'], r'^--look teal: mono or sepia$'), (['--look', 'Mono'], r'^--look Mono: mono or sepia$'),
        (['--look', 'mono', '--lut-strength', '0'], r'^--lut-strength 0: above 0 and at most 1$'), (['--look', 'mono', '--lut-strength', '1.01'], r'^--lut-strength 1\.01: above 0 and at most 1$'),
        (['--look', 'mono', '--lut-strength', '-0.5'], r'^--lut-strength -0\.5: '), (['--look', 'mono', '--lut-strength', 'half'], r'^--lut-strength half: '),
        (['--look', 'mono', '--lut-strength', 'nan'], r'^--lut-strength nan: '), (['--look', 'mono', '--lut-strength', '0.001'], r'^--lut-strength 0\.001: '),
        (['--lut-strength', '0.5'], r'^--lut-strength 0\.5: only with --lut, --grade or --look$'))


def _stopping_pipeline(monkeypatch):
    from ken_burns_effect_amd import pipeline
    built = []

    class Stop(Exception):
        pass

    def init(self, *a, **k):
        built.append(k)
        raise Stop()
    monkeypatch.setattr(pipeline.Pipeline, '__init__', init)
    return built, Stop


def test_kbe_refuses_before_a_network_is_built(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import grade, kbe
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    built, Stop = _stopping_pipeline(monkeypatch)
    P = _files(tmp_path)
    photo, out = str(tmp_path / 'in.png'), str(tmp_path / 'out')
    Image.fromarray(gif_cases.photo_like(48, 64, 1)).save(photo)
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        for argv, text in _refusals(P):
            with pytest.raises(SystemExit, match=text):
                kbe.main(['--in', photo, '--out', out] + argv)
        assert built == [] and not os.path.exists(out)
        # what is in order reaches the Pipeline, as it was given
        for argv in (['--lut', P['good'], '--grade', 'contrast=1.2, gamma=0.9', '--look', 'sepia', '--lut-strength', '0.5'], ['--grade', 'brightness=4,contrast=0,saturation=4,gamma=10'],
                     ['--look', 'mono'], []):
            with pytest.raises(Stop):
                kbe.main(['--in', photo, '--out', out] + argv)
        with pytest.warns(UserWarning, match=r'^--lut .*big\.cube: its table of 35 nodes per axis is resampled to 33'):
            request = kbe.parse(['--lut', P['big']])[0]['graded']
        assert request['table'].shape == (33, 33, 33, 3) and request['strength'] == 256
        # the environment's twins
        monkeypatch.setenv('KBE_LUT', P['short'])
        with pytest.raises(SystemExit, match=r'^--lut .*short\.cube: line \d+: 7 rows'):
            kbe.main(['--in', photo, '--out', out])
        monkeypatch.setenv('KBE_LUT', P['good'])
        monkeypatch.setenv('KBE_GRADE', 'saturation=0.5')
        monkeypatch.setenv('KBE_LOOK', 'mono')
        monkeypatch.setenv('KBE_LUT_STRENGTH', '0.25')
        request = kbe.parse([])[0]['graded']
        assert (request['lut'], request['grade'], request['look'], request['strength']) == (P['good'], {'saturation': 0.5}, 'mono', 64) and request['table'].shape == (33, 33, 33, 3)
        assert kbe.parse(['--look', 'sepia', '--lut-strength', '1'])[0]['graded']['look'] == 'sepia' and kbe.parse(['--lut-strength', '1'])[0]['graded']['strength'] == 256
    finally:
        torch.set_grad_enabled(grad)
    assert len(built) == 4 and not os.path.exists(out)
    assert (built[0]['lut'], built[0]['grade'], built[0]['look'], built[0]['lut_strength']) == (P['good'], 'contrast=1.2, gamma=0.9', 'sepia', '0.5')
    assert all(built[3][name] is None for name in grade.OPTIONS) and set(grade.OPTIONS) <= set(built[3])
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    # the finished grade: --grade and --look first, then the file's table; a file alone at its own size
    assert grade.grade_request() is None and grade.grade_for(None) is None
    alone = grade.grade_request(lut=P['good'])
    assert alone['table'].shape == (4, 4, 4, 3) and np.array_equal(alone['table'], grade.read_cube(P['good'])) and grade.grade_for(alone, True)[0].shape == (4, 4, 4)
    both = grade.grade_request(lut=P['good'], grade={'contrast': 1.2}, look='mono', lut_strength=0.75)
    assert np.allclose(both['table'], grade.compose(grade.bake(contrast=1.2, look='mono'), grade.read_cube(P['good']))) and both['strength'] == 192
    assert not np.allclose(both['table'], grade.compose(grade.resample(grade.read_cube(P['good']), 33), grade.bake(contrast=1.2, look='mono')), atol=1e-3)      # (the other order)
    table, strength = grade.grade_for(grade.grade_request(look='sepia'), False)
    assert strength == 256 and np.array_equal(table, grade.quantise(grade.bake(look='sepia'), False)) and not np.array_equal(table, grade.grade_for(grade.grade_request(look='sepia'), True)[0])
    assert '--lut FILE' in kbe.__doc__ and '--look mono|sepia' in kbe.__doc__ and 'KBE_LUT_STRENGTH' in kbe.__doc__


def test_the_slideshow_refuses_before_a_network_is_built(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import slideshow
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    built, Stop = _stopping_pipeline(monkeypatch)
    P = _files(tmp_path)
    photos, out = [str(tmp_path / ('in%d.png' % k)) for k in range(2)], str(tmp_path / 'out')
    for k, path in enumerate(photos):
        Image.fromarray(gif_cases.photo_like(48, 64, 1 + k)).save(path)
    grad = torch.is_grad_enabled()
    try:
        for argv, text in _refusals(P):
            with pytest.raises(SystemExit, match=text):
                slideshow.main(['--in', photos[0], '--in', photos[1], '--out', out] + argv)
        assert built == [] and not os.path.exists(out)
        for argv in (['--lut', P['good'], '--look', 'sepia', '--lut-strength', '0.5'], ['--grade', 'gamma=2.2'], []):
            with pytest.raises(Stop):
                slideshow.main(['--in', photos[0], '--in', photos[1], '--out', out] + argv)
    finally:
        torch.set_grad_enabled(grad)
    # the slideshow's Pipeline is built with the grade: its render grades every clip
    assert len(built) == 3 and not os.path.exists(out)
    assert (built[0]['lut'], built[0]['grade'], built[0]['look'], built[0]['lut_strength']) == (P['good'], None, 'sepia', '0.5') and built[1]['grade'] == 'gamma=2.2'
    assert all(built[2][name] is None for name in ('lut', 'grade', 'look', 'lut_strength'))
    assert all(name + '=' in slideshow.LONG_OPTIONS for name in ('lut', 'grade', 'look', 'lut-strength')) and '--lut FILE' in slideshow.__doc__


def test_the_pipeline_refuses_before_a_network_runs(tmp_path, monkeypatch):
    """Pipeline._run and Pipeline.render look at the grade before estimate(): on a bare instance whose estimate raises, every refusal comes
    first, and what is in order reaches estimate; slideshow.make refuses before its first render."""
    import torch
    from ken_burns_effect_amd import pipeline, slideshow
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    P = _files(tmp_path)

    class Reached(Exception):
        pass

    def estimate(self, image):
        raise Reached()
    monkeypatch.setattr(pipeline.Pipeline, 'estimate', estimate)
    pipe = object.__new__(pipeline.Pipeline)
    pipe.device, pipe.steps, pipe.dolly, pipe.output_frames, pipe.miopen_find, pipe.partial_inpainting = torch.device('cpu'), 6, False, False, False, False
    image = torch.zeros(1, 3, 48, 64)
    zoom = {'objectFrom': {'dblCenterU': 32, 'dblCenterV': 24, 'intCropWidth': 56, 'intCropHeight': 42}, 'objectTo': {'dblCenterU': 32, 'dblCenterV': 24, 'intCropWidth': 48, 'intCropHeight': 36}}
    refusals = ((dict(lut=P['none']), r'^--lut .*none\.cube: no such file$'), (dict(lut=P['one']), r'^--lut .*one\.cube: line 1: LUT_1D_SIZE'), (dict(grade='hue=2'), r'^--grade hue=2: unknown key hue'),
                (dict(grade={'gamma': 20}), r'^--grade .*gamma=20: 0\.1\.\.10$'), (dict(look='warm'), r'^--look warm: mono or sepia$'), (dict(look='mono', lut_strength=0), r'^--lut-strength 0: '),
                (dict(lut_strength=0.5), r'^--lut-strength 0\.5: only with --lut, --grade or --look$'))
    for options, text in refusals:
        for name in ('lut', 'grade', 'look', 'lut_strength'):
            setattr(pipe, name, options.get(name))
        for call in (lambda: pipe(image, zoom, str(tmp_path / 'out')), lambda: pipe.render(image, zoom), lambda: slideshow.make([image, image], str(tmp_path / 'out'), pipe, 'dissolve', 2)):
            with pytest.raises(ValueError, match=text):
                call()
    for options in (dict(lut=P['good'], grade={'contrast': 1.1}, look='sepia', lut_strength=0.5), dict(look='mono'), dict()):
        for name in ('lut', 'grade', 'look', 'lut_strength'):
            setattr(pipe, name, options.get(name))
        for call in (lambda: pipe(image, zoom, str(tmp_path / 'out')), lambda: pipe.render(image, zoom)):
            with pytest.raises(Reached):
                call()
    monkeypatch.setenv('KBE_LOOK', 'warm')
    with pytest.raises(ValueError, match=r'^--look warm: mono or sepia$'):
        pipe(image, zoom, str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists()
    monkeypatch.delenv('KBE_LOOK')
    assert pipeline.grade_of(type('Bare', (), {})()) is None and pipeline.with_grade(None, image) is image
