"""The depth-of-field blur (include/kbe_dof.h) without a GPU: csrc/kbe_dof_block.h executed serially (tests/dof_check.cpp) against a restatement
that scatters and against the NumPy twin (tests/dof_cases.py); the properties that follow from the definition; the radius rule at its
thresholds; the focus helpers; the binding (dof.py) held to what tests/test_header_bindings.py holds the older headers to; every refusal of
the entry on host memory; and the command line's --aperture / --focus / --focus-to and Pipeline(aperture=, focus=, focus_to=)."""
import ctypes
import inspect
import os
import re
from ctypes import c_double, c_int, c_void_p

import numpy as np
import pytest
from PIL import Image

import dof_cases as dc
import gif_cases as gc
import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition ---------------------------------------------------------------------------
def test_the_header_against_the_scatter_restatement():
    """dof_check.cpp builds; the table is the issue's list; the sums fit 32 bits; and gather_pixel equals the scatter restatement at every frame
    size up to 7 x 7 with R in {0, 1, 2, 3} and three apertures (49 * 4 * 3 cases) and at 40 x 24 with R = 16."""
    m = re.search(r'brute: cases (\d+), blurred pixels (\d+), mismatches (\d+), bad table entries (\d+), sums fit 32 bits: (\w+) \(2 sum\(wv\) \+ sum\(w\) <= (\d+)\)', dc.ask('brute'))
    cases, blurred, mismatches, bad_table, fits, bound = m.groups()
    assert int(cases) == 49 * 4 * 3 + 1 and int(blurred) > 1000 and int(mismatches) == 0 and int(bad_table) == 0 and fits == 'yes' and int(bound) < 2 ** 32


def test_the_table_is_the_issues():
    assert [dc.disc_points(e) for e in range(17)] == dc.DISC
    assert dc.WEIGHT.tolist() == [8192, 1638, 630, 282, 167, 101, 72, 54, 41, 32, 25, 21, 18, 15, 13, 11, 10]
    assert 2 * 255 * (8192 + 1088 * 1638) + (8192 + 1088 * 1638) < 2 ** 32


@pytest.mark.parametrize('R', dc.RADII)
@pytest.mark.parametrize('frame', dc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_header_is_the_twin(frame, R):
    """gather_pixel of csrc/kbe_dof_block.h on the GPU suite's frames and depths, rows padded: the NumPy twin byte for byte; two frames whose
    focus depths differ."""
    W, H = frame
    got = dc.header_blur(dc.frames(W, H), dc.depths(W, H), dc.focus_of(2), dc.APERTURE, R, pad=5, z_pad=3)
    assert np.array_equal(got, dc.twin_of(W, H, R))


def test_the_cases_reach_every_radius_and_blur():
    for W, H in dc.FRAMES:
        r = dc.twin_radius(dc.depths(W, H)[0], dc.FOCUS[0], dc.APERTURE, 16)
        assert r.min() == 0 and r.max() == 16 and len(np.unique(r)) >= 10
        assert (dc.twin_of(W, H, 16) != dc.frames(W, H)).mean() > 0.3 and np.array_equal(dc.twin_of(W, H, 0), dc.frames(W, H))
        assert not np.array_equal(dc.twin_of(W, H, 5), dc.twin_of(W, H, 16))


# -- the radius ---------------------------------------------------------------------------------
def test_the_radius_at_its_thresholds():
    """z = 64, zf = 96: t = 32 and the right sides are 32 (2 j - 1), so A = 2 j - 1 makes A t exactly (j - 0.5) z: that counts, and A one ulp
    below does not.  The twin and the header agree."""
    z = np.full(16, 64.0, np.float32)
    for j in range(1, 17):
        A = np.float32(2 * j - 1)
        below = np.nextafter(A, np.float32(0.0), dtype=np.float32)
        assert np.float32(A * np.float32(32.0)) == np.float32(j - 0.5) * np.float32(64.0) and below < A
        for twin in (dc.twin_radius, dc.header_radius):
            assert (twin(z, 96.0, A, 16) == j).all() and (twin(z, 96.0, below, 16) == j - 1).all(), (j, twin.__name__)
            assert (twin(z, 96.0, A, min(j + 2, 16)) == j).all() and (twin(z, 96.0, A, j - 1) == j - 1).all()           # the cap


def test_the_radius_is_the_rounded_quotient_away_from_its_ties():
    rng = np.random.RandomState(3)
    z = rng.uniform(20.0, 900.0, 4000).astype(np.float32)
    for zf, A in ((120.0, 20.0), (300.0, 7.5), (55.0, 40.0)):
        q = A * np.abs(z.astype(np.float64) - zf) / z.astype(np.float64)
        clear = np.abs(q - np.floor(q) - 0.5) > 1e-4
        want = np.minimum(16, np.floor(q + 0.5)).astype(np.int64)
        got = dc.twin_radius(z, zf, A, 16)
        assert clear.sum() > 3900 and np.array_equal(got[clear], want[clear]) and np.array_equal(got, dc.header_radius(z, zf, A, 16))


def test_the_specials_give_radius_0():
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -5.0, -1e30], np.float32)
    for A in (0.0, 20.0, 1e30):
        assert (dc.twin_radius(specials, 120.0, A, 16) == 0).all() and (dc.header_radius(specials, 120.0, A, 16) == 0).all()
    # (and beside them ordinary depths keep theirs; a product that overflows to +inf still compares)
    mixed = np.array([np.nan, 60.0, np.inf, 3e38, 1e-30], np.float32)
    assert dc.twin_radius(mixed, 120.0, 20.0, 16).tolist() == dc.header_radius(mixed, 120.0, 20.0, 16).tolist() == [0, 16, 0, 16, 16]
    assert dc.twin_radius(mixed, 120.0, 1e38, 16).tolist() == dc.header_radius(mixed, 120.0, 1e38, 16).tolist() == [0, 16, 0, 16, 16]


def test_the_radius_of_subnormal_depths():
    """Depths and a focus below the smallest normal fp32 number are valid (z > 0, finite) and nothing flushes them: every operation is still one
    IEEE rounding, so zf = 1e-40 and A = 3 give z = 3e-40, 1.5e-40 and 2.5e-40 the radii round(3 (z - zf) / z) = 2, 1, 2; the smallest normal
    number gets 3.  The twin and the header agree; a build that flushed them to zero would give 0 (z = 0 is no depth)."""
    z = np.array([3e-40, 1.5e-40, 2.5e-40, 1.1754944e-38], np.float32)
    assert (z > 0).all() and (z[:3] < np.finfo(np.float32).tiny).all() and z[3] == np.finfo(np.float32).tiny and 0 < np.float32(1e-40) < z.min()
    for A, want in ((3.0, [2, 1, 2, 3]), (1.0, [1, 0, 1, 1]), (20.0, [13, 7, 12, 16])):
        assert dc.twin_radius(z, 1e-40, A, 16).tolist() == dc.header_radius(z, 1e-40, A, 16).tolist() == want, A
    # a subnormal depth against a normal focus, and a normal depth against a subnormal focus
    assert dc.twin_radius(z, 120.0, 20.0, 16).tolist() == dc.header_radius(z, 120.0, 20.0, 16).tolist() == [16] * 4
    assert dc.twin_radius(np.array([64.0], np.float32), 1e-40, 7.0, 16).tolist() == dc.header_radius(np.array([64.0], np.float32), 1e-40, 7.0, 16).tolist() == [7]


# -- the properties that follow -------------------------------------------------------------------
def test_no_aperture_no_radius_or_everything_in_focus_returns_the_frame():
    W, H = dc.FRAMES[0]
    frames, depths = dc.frames(W, H), dc.depths(W, H)
    assert np.array_equal(dc.twin_blur(frames, depths, dc.focus_of(2), 0.0, 16), frames)
    assert np.array_equal(dc.twin_blur(frames, depths, dc.focus_of(2), dc.APERTURE, 0), frames)
    level = np.full((2, H, W), 77.5, np.float32)
    assert np.array_equal(dc.twin_blur(frames, level, [77.5, 77.5], 1e6, 16), frames)
    assert np.array_equal(dc.header_blur(frames, level, [77.5, 77.5], 1e6, 16), frames) and np.array_equal(dc.header_blur(frames, depths, dc.focus_of(2), 0.0, 16), frames)


def test_a_frame_of_one_colour_stays_that_colour():
    W, H = dc.FRAMES[0]
    depths = np.array(dc.depths(W, H))
    depths[0, ::7, ::5] = np.nan
    depths[1, 3::9, 1::4] = -5.0
    for value in (0, 1, 137, 254, 255):
        frames = np.full((2, H, W, 3), value, np.uint8)
        assert (dc.twin_blur(frames, depths, dc.focus_of(2), dc.APERTURE, 16) == value).all()
    mixed = np.empty((2, H, W, 3), np.uint8)
    mixed[:] = (3, 200, 255)
    assert (dc.header_blur(mixed, depths, dc.focus_of(2), dc.APERTURE, 16) == np.array([3, 200, 255], np.uint8)).all()


def _edge(near_radius, far_radius, H=41, W=60):
    """Left half: colour 30 at depth 50; right half: colour 220 at depth 100; the focus and the aperture chosen so that the halves get these radii."""
    frame = np.empty((1, H, W, 3), np.uint8)
    frame[:, :, :W // 2], frame[:, :, W // 2:] = 30, 220
    depth = np.empty((1, H, W), np.float32)
    depth[:, :, :W // 2], depth[:, :, W // 2:] = 50.0, 100.0
    if near_radius == 0:
        focus, A = 50.0, 2.0 * far_radius          # A |100 - 50| / 100
    else:
        focus, A = 100.0, float(near_radius)       # A |50 - 100| / 50
    r = dc.twin_radius(depth[0], focus, A, 16)
    assert (r[:, :W // 2] == near_radius).all() and (r[:, W // 2:] == far_radius).all()
    return frame, depth, focus, A


def test_a_sharp_foreground_before_a_blurred_background_keeps_both_sides():
    frame, depth, focus, A = _edge(0, 8)
    assert np.array_equal(dc.twin_blur(frame, depth, [focus], A, 16), frame) and np.array_equal(dc.header_blur(frame, depth, [focus], A, 16), frame)


def test_a_blurred_foreground_spills_over_a_sharp_background():
    frame, depth, focus, A = _edge(8, 0)
    got = dc.twin_blur(frame, depth, [focus], A, 16)
    assert np.array_equal(got, dc.header_blur(frame, depth, [focus], A, 16))
    assert np.array_equal(got[:, :, :30], frame[:, :, :30])                      # the foreground side keeps its bytes
    row = got[0, 20, 30:, 0].tolist()                                            # a row 20 pixels from the frame's top and bottom
    assert row[:3] == [161, 168, 176] and row[7] == 219 and row[8:] == [220] * 22 and row[:9] == sorted(row[:9]) and len(set(row[:9])) == 9
    assert (got[0, 20] == got[0, 20, :, :1]).all()                               # channels alike


def test_a_frames_bytes_do_not_depend_on_its_neighbours():
    W, H = dc.FRAMES[0]
    frames, depths, focus = dc.frames(W, H, 3), dc.depths(W, H, 3), dc.focus_of(3)
    together = dc.twin_blur(frames, depths, focus, dc.APERTURE, 5)
    for i in range(3):
        assert np.array_equal(dc.twin_blur(frames[i:i + 1], depths[i:i + 1], focus[i:i + 1], dc.APERTURE, 5)[0], together[i])
    assert not np.array_equal(dc.twin_blur(frames[:1], depths[:1], [focus[1]], dc.APERTURE, 5)[0], together[0])             # the focus matters


# -- the focus helpers ------------------------------------------------------------------------------
def test_focus_path():
    from ken_burns_effect_amd import dof
    for z0, z1, steps in ((100.0, 50.0, 5), (37.3, 911.7, 75), (640.0, 640.0, 3), (0.1, 1e6, 12)):
        path = dof.focus_path(z0, z1, steps)
        assert len(path) == steps and path[0] == z0 and path[-1] == z1
        inverse = np.array([1.0 / z for z in path])
        steps_of = np.diff(inverse)
        assert (steps_of <= 0).all() if z0 <= z1 else (steps_of >= 0).all()                                    # monotone in 1 / z
        assert np.allclose(steps_of, (1.0 / z1 - 1.0 / z0) / (steps - 1), rtol=1e-9, atol=1e-18)               # and linear in it
    assert dof.focus_path(100.0, 50.0, 5) == [100.0, 80.0, 1.0 / (0.01 + 0.005), 1.0 / (0.01 + 0.0075), 50.0]
    assert dof.focus_path(12.5, 99.0, 1) == [12.5]
    for bad in ((0.0, 5.0, 3), (5.0, -1.0, 3), (float('nan'), 5.0, 3), (5.0, float('inf'), 3), (5.0, 6.0, 0)):
        with pytest.raises(ValueError, match='focus_path'):
            dof.focus_path(*bad)


def test_focus_depth_is_the_median_of_5_x_5_clamped_to_the_image():
    import torch
    from ken_burns_effect_amd import dof
    H, W = 9, 11
    plane = np.random.RandomState(5).uniform(10.0, 500.0, (H, W)).astype(np.float32)
    depth = torch.from_numpy(plane).reshape(1, 1, H, W)

    def want(x, y):
        xs, ys = np.clip(np.arange(x - 2, x + 3), 0, W - 1), np.clip(np.arange(y - 2, y + 3), 0, H - 1)
        return float(np.sort(plane[np.ix_(ys, xs)].reshape(-1))[12])
    for u, v, (x, y) in ((5, 4, (5, 4)), (0, 0, (0, 0)), (10, 8, (10, 8)), (0, 8, (0, 8)), (10, 0, (10, 0)), (4.4, 3.6, (4, 4)), (4.5, 3.5, (5, 4)), (1, 7, (1, 7))):
        assert dof.focus_depth(depth, u, v) == want(x, y), (u, v)
    plane[:] = 80.0
    plane[4, 5] = 1e9                                                          # (a median: one wild depth under the point does not move it)
    assert dof.focus_depth(torch.from_numpy(plane).reshape(1, 1, H, W), 5, 4) == 80.0


def test_the_lens_is_a_small_record_and_is_checked():
    from ken_burns_effect_amd import dof
    assert dof.Lens(100.0, 50.0, 6.0) == (100.0, 50.0, 6.0, 16) and dof.Lens(1, 2, 3, 4).max_radius == 4 and dof.MAX_RADIUS == 16
    assert dof.checked_lens((100, 50, 6)) == dof.Lens(100.0, 50.0, 6.0, 16)
    for bad in ((0.0, 50.0, 6.0), (100.0, float('nan'), 6.0), (100.0, 50.0, -1.0), (100.0, 50.0, float('inf')), (100.0, 50.0, 6.0, 17), (100.0, 50.0, 6.0, -1), (100.0, 50.0, 6.0, 2.5)):
        with pytest.raises(ValueError, match='^lens: '):
            dof.checked_lens(bad)


# -- the binding -------------------------------------------------------------------------------
p, i, d = c_void_p, c_int, c_double
NULL_CALL = (None, None, 1, 4, 4, 12, 4, None, 1.0, 4, None, 12, None)
DOF = thb.Binding(
    'dof', 'kbe_dof',
    # frames, depths, n, W, H, stride, depth stride; focus, aperture, max radius; out, out stride; stream
    {'kbe_dof_abi_version': (c_int, []), 'kbe_dof_u8': (c_int, [p, p, i, i, i, i, i, p, d, i, p, i, p])},
    'kbe_dof_abi_version', ['#define KBE_DOF_ABI_VERSION 1\n'], ['KBE_DOF_BGR'], {'ABI_VERSION': 1, 'MAX_RADIUS': 16},
    [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
     ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n')],
    ('kbe_dof_u8', NULL_CALL, 'kbe_dof_u8: null frames_u8'),
    ('kbe_dof_u8', None, lambda frames: ((frames, frames, 1.0, 4, 4, 12, 4, frames, 1.0, 4, frames, 12, None), (frames, frames, 1, 4, 4, 12, 4, frames, 'wide', 4, frames, 12, None),
                                         (frames, frames, 1, 4, 4, 12, 4, frames, 1.0, 4, frames, 12))),
    [('kbe_dof_abi_version', 0, (1,)), ('kbe_dof_u8', 13, NULL_CALL + (0,)), ('kbe_dof_u8', 13, NULL_CALL[:-1])],
    ['kbe_crop_area_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_dof_u8', lambda at: ((c_void_p * 2)(at, at + 1024), (c_void_p * 2)(at + 2048, at + 3200), 2, 16, 17, 48, 16, (c_double * 2)(1.0, 2.0), 1.0, 17,
                               (c_void_p * 2)(at + 4352, at + 5376), 48, None),
     'kbe_dof_u8 failed (-1): kbe_dof_u8: max_radius outside 0..16'),
    ['kbe_dof_u8'], set())


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(DOF)


def test_the_library_exports_them_beside_the_others():
    thb.test_the_library_exports_them_with_the_headers_types(DOF)
    from ken_burns_effect_amd import _native, crop_area, dof
    lib = dof.load()
    assert lib is _native.load() is crop_area.load() and lib.kbe_dof_abi_version() == 1 == dof.ABI_VERSION and lib.kbe_crop_area_abi_version() == 1
    for older in thb.BINDINGS:
        assert getattr(thb.module_of(older).load(), older.abi)() == 1 and thb.module_of(older).load() is lib


def test_the_older_headers_and_their_bindings_are_what_they_were():
    from ken_burns_effect_amd import _native, crop_area, dof
    b = DOF
    dof.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    with open(_native.__file__) as f:
        assert b.prefix not in f.read()
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for other in [thb.module_of(older) for older in thb.BINDINGS] + [crop_area]:
        assert not any(name.startswith(b.prefix) for name in other.prototypes())
        with open(other.__file__) as f:
            assert b.prefix not in f.read()
    assert list(crop_area.prototypes()) == ['kbe_crop_area_abi_version', 'kbe_crop_area_u8']
    # this is the only module of the package that names the entry
    package = os.path.dirname(dof.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and 'kbe_dof_u8' in open(os.path.join(package, name)).read()]
    assert naming == ['dof.py']
    name, args, text = b.null_call
    assert dof._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(DOF)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(DOF)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(DOF)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(DOF)


# (frames of 16 x 17 at a stride of 48: 816 bytes; depth planes at a stride of 16 floats: 1088 bytes)
REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null depths': (dict(depth_f32=None), 'null depth_f32'), 'null focus': (dict(focus=None), 'null focus'),
           'null out': (dict(out_u8=None), 'null out_u8'), 'n = 0': (dict(n_frames=0), 'n_frames < 1'), 'W = 0': (dict(W=0), 'W or H outside 1..65535'),
           'H = 65536': (dict(H=65536), 'W or H outside 1..65535'), 'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'), 'depth stride': (dict(depth_stride_floats=15), 'depth_stride_floats < W'),
           'out stride': (dict(out_stride_bytes=47), 'out_stride_bytes < 3 W'), 'radius 17': (dict(max_radius=17), 'max_radius outside 0..16'), 'radius -1': (dict(max_radius=-1), 'max_radius outside 0..16'),
           'aperture -1': (dict(aperture=-1.0), 'aperture is not a finite number >= 0'), 'aperture nan': (dict(aperture=float('nan')), 'aperture is not a finite number >= 0'),
           'aperture inf': (dict(aperture=float('inf')), 'aperture is not a finite number >= 0'), 'aperture 1e300': (dict(aperture=1e300), 'aperture is not a finite number >= 0'),
           'null frame 1': (dict(frames_u8=1), 'null element of frames_u8'), 'null plane 1': (dict(depth_f32=1), 'null element of depth_f32'), 'null output 1': (dict(out_u8=1), 'null element of out_u8'),
           'focus 0': (dict(focus=0.0), 'an element of focus is not a finite number > 0'), 'focus -3': (dict(focus=-3.0), 'an element of focus is not a finite number > 0'),
           'focus nan': (dict(focus=float('nan')), 'an element of focus is not a finite number > 0'), 'focus inf': (dict(focus=float('inf')), 'an element of focus is not a finite number > 0'),
           'focus 1e-60': (dict(focus=1e-60), 'an element of focus is not a finite number > 0'),
           # (the frames lie at 0 and 2048, the depth planes at 8192 and 9472, the outputs at 4096 and 5120; (a, b): outputs moved there, None: as it was)
           'in place': (dict(out_u8=(0, None)), 'an element of out_u8 overlaps a source frame'), 'onto the other frame': (dict(out_u8=(2048, None)), 'an element of out_u8 overlaps a source frame'),
           'one byte into the next source': (dict(out_u8=(2048 - 815, None)), 'an element of out_u8 overlaps a source frame'),
           'the last byte of the last source': (dict(out_u8=(None, 2048 + 815)), 'an element of out_u8 overlaps a source frame'),
           'the last byte of a depth plane': (dict(out_u8=(None, 9472 + 1087)), 'an element of out_u8 overlaps a depth plane')}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, dof
    memory = (ctypes.c_uint64 * 2048)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 2)(at, at + 2048), depth_f32=(c_void_p * 2)(at + 8192, at + 9472), n_frames=2, W=16, H=17, stride_bytes=48, depth_stride_floats=16,
                focus=(c_double * 2)(100.0, 50.0), aperture=6.0, max_radius=16, out_u8=(c_void_p * 2)(at + 4096, at + 5120), out_stride_bytes=48, stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key in ('frames_u8', 'depth_f32', 'out_u8') and value == 1:
            args[key][1] = None
        elif key == 'out_u8' and isinstance(value, tuple):
            for k in (0, 1):
                if value[k] is not None:
                    args[key][k] = at + value[k]
        elif key == 'focus' and value is not None:
            args[key][1] = value
        else:
            args[key] = value
    assert dof._raw('kbe_dof_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_dof_u8: ' + text
    assert not any(memory)


def test_apply_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, dof
    with pytest.raises(_native.KbeError):
        dof.apply(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.ones(1, 8, 8), [1.0], 2.0)


# -- the command line and Pipeline ---------------------------------------------------------------
def test_the_command_line_takes_and_refuses_the_lens(monkeypatch):
    from ken_burns_effect_amd import kbe
    for name in ('KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO'):
        monkeypatch.delenv(name, raising=False)
    cfg = kbe.parse([])[0]
    assert cfg['aperture'] is None and cfg['focus'] is None and cfg['focus-to'] is None
    cfg = kbe.parse(['--aperture', '6.5', '--focus', '10,20', '--focus-to', '300.5,7', '--width', '64', '--gif', '--dolly'])[0]
    assert cfg['aperture'] == 6.5 and cfg['focus'] == (10.0, 20.0) and cfg['focus-to'] == (300.5, 7.0) and cfg['width'] == 64 and cfg['gif'] and cfg['dolly']
    assert kbe.parse(['--aperture', '6'])[0]['aperture'] == 6.0 and kbe.parse(['--aperture', '6'])[0]['focus'] is None
    for argv, text in ((['--focus', '10,20'], r'^--focus 10,20: only with --aperture$'), (['--focus-to', '1,2'], r'^--focus-to 1,2: only with --aperture$'),
                       (['--aperture', '0'], r'^--aperture 0: the aperture \(KBE_APERTURE, --aperture\): pixels, a finite number above 0$'), (['--aperture', 'nan'], 'a finite number above 0'),
                       (['--aperture', '-1'], r'^--aperture -1: the aperture'), (['--aperture', 'inf'], 'a finite number above 0'), (['--aperture', 'wide'], 'a finite number above 0'),
                       (['--aperture', '4', '--focus', '12'], r'^--focus 12: U,V, a pixel of the photo$'), (['--aperture', '4', '--focus-to', 'a,b'], r'^--focus-to a,b: U,V, a pixel of the photo$')):
        with pytest.raises(SystemExit, match=text):
            kbe.parse(argv)


def test_lens_request_and_lens_points(monkeypatch):
    from ken_burns_effect_amd import pipeline, synthetic
    for name in ('KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO'):
        monkeypatch.delenv(name, raising=False)
    assert pipeline.lens_request() is None and pipeline.lens_request(6) == (6.0, None, None) and pipeline.lens_request('2.5', '3,4', (5, 6)) == (2.5, (3.0, 4.0), (5.0, 6.0))
    for bad in (0, -1, float('nan'), float('inf'), 'wide', '0'):
        with pytest.raises(ValueError, match=r'^the aperture \(KBE_APERTURE, --aperture\): pixels, a finite number above 0$'):
            pipeline.lens_request(bad)
    with pytest.raises(ValueError, match=r'^focus \(KBE_FOCUS, --focus\): only with an aperture \(KBE_APERTURE, --aperture\)$'):
        pipeline.lens_request(None, (3, 4))
    with pytest.raises(ValueError, match=r'^focus_to \(KBE_FOCUS_TO, --focus-to\): only with an aperture'):
        pipeline.lens_request(None, None, '3,4')
    monkeypatch.setenv('KBE_FOCUS', '7,8')
    with pytest.raises(ValueError, match='only with an aperture'):
        pipeline.lens_request()
    monkeypatch.setenv('KBE_APERTURE', '12')
    monkeypatch.setenv('KBE_FOCUS_TO', '9,10.5')
    assert pipeline.lens_request() == (12.0, (7.0, 8.0), (9.0, 10.5)) and pipeline.lens_request(3, (1, 2)) == (3.0, (1.0, 2.0), (9.0, 10.5))
    monkeypatch.setenv('KBE_APERTURE', 'nan')
    with pytest.raises(ValueError, match='KBE_APERTURE'):
        pipeline.lens_request()
    # the points: the default focus is the centre of the end window, the default focus_to the focus; a point outside the image is refused
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    centre = (float(oto['dblCenterU']), float(oto['dblCenterV']))
    assert pipeline.lens_points(None, 64, 48, zoom) is None
    assert pipeline.lens_points((6.0, None, None), 64, 48, zoom) == (6.0, centre, centre) and 0 < centre[0] < 63 and 0 < centre[1] < 47
    assert pipeline.lens_points((6.0, (1.0, 2.0), None), 64, 48, zoom) == (6.0, (1.0, 2.0), (1.0, 2.0))
    assert pipeline.lens_points((6.0, None, (63.0, 47.0)), 64, 48, zoom) == (6.0, centre, (63.0, 47.0))
    for points, text in ((((5000.0, 10.0), None), r'^focus 5000,10: the image is 64x48: a pixel of the photo, 0\.\.63 and 0\.\.47$'), (((10.0, 48.0), None), '^focus 10,48: '),
                         (((-1.0, 3.0), None), '^focus -1,3: '), ((None, (64.0, 3.0)), '^focus_to 64,3: the image is 64x48')):
        with pytest.raises(ValueError, match=text):
            pipeline.lens_points((6.0,) + points, 64, 48, zoom)


def _stub(P, calls, **settings):
    import torch

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = False, False, 2, {}, None, torch.device('cpu')
            for name, value in settings.items():
                setattr(self, name, value)

        def estimate(self, tensorImage):
            calls.append('estimate')
            raise AssertionError('a network ran')
    return Stub()


def test_a_lens_that_cannot_be_is_refused_before_a_network_runs(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import kbe, pipeline, synthetic
    for name in ('KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_WIDTH', 'KBE_GIF'):
        monkeypatch.delenv(name, raising=False)
    calls = []
    monkeypatch.setattr(pipeline.common, 'process_kenburns', lambda *a, **k: calls.append('render'))
    image = torch.zeros(1, 3, 48, 64)
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    for settings, text in ((dict(focus=(3, 4)), 'only with an aperture'), (dict(focus_to='3,4'), 'only with an aperture'), (dict(aperture=0), 'a finite number above 0'),
                           (dict(aperture=float('nan')), 'a finite number above 0'), (dict(aperture=-1), 'a finite number above 0'),
                           (dict(aperture=6, focus=(5000, 10)), '^focus 5000,10: the image is 64x48'), (dict(aperture=6, focus_to=(10, 48)), '^focus_to 10,48: the image is 64x48')):
        with pytest.raises(ValueError, match=text):
            _stub(pipeline, calls, **settings)(image, zoom, str(tmp_path / 'out'))
    monkeypatch.setenv('KBE_FOCUS', '3,4')
    with pytest.raises(ValueError, match='only with an aperture'):
        _stub(pipeline, calls)(image, zoom, None)
    monkeypatch.setenv('KBE_APERTURE', '0')
    with pytest.raises(ValueError, match='a finite number above 0'):
        _stub(pipeline, calls)(image, zoom, None)
    assert calls == [] and not (tmp_path / 'out').exists()
    # the command line: before Pipeline is built
    monkeypatch.delenv('KBE_FOCUS')
    monkeypatch.delenv('KBE_APERTURE')
    built = []
    monkeypatch.setattr(pipeline.Pipeline, '__init__', lambda self, *a, **k: built.append(k))
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(48, 64, 1)).save(path)
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        with pytest.raises(SystemExit, match=r'^--focus 5000,10: the image is 64x48: a pixel of the photo, 0\.\.63 and 0\.\.47$'):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--aperture', '6', '--focus', '5000,10'])
        with pytest.raises(SystemExit, match=r'^--focus-to 10,48: the image is 64x48'):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--aperture', '6', '--focus-to', '10,48'])
        with pytest.raises(SystemExit, match=r'^--focus 10,20: only with --aperture$'):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--focus', '10,20'])
        with pytest.raises(SystemExit, match=r'^--aperture 0: '):
            kbe.main(['--in', path, '--out', str(tmp_path / 'out'), '--aperture', '0'])
    finally:
        torch.set_grad_enabled(grad)
    assert built == [] and not (tmp_path / 'out').exists()


def test_the_pipeline_passes_a_lens_only_when_there_is_an_aperture(monkeypatch):
    """Without an aperture process_kenburns is called with exactly the arguments it had; with one, the lens holds the median depths at the two
    focus points, read from the estimated depth, and combines with a width."""
    import torch
    from ken_burns_effect_amd import dof, pipeline, synthetic
    for name in ('KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_PNG', 'KBE_JPEG'):
        monkeypatch.delenv(name, raising=False)
    seen = []

    def kenburns(*args, **kw):
        seen.append(kw)
        size = kw.get('out_size', (64, 48))
        return [np.zeros((size[1], size[0], 3), np.uint8) for _ in range(2)]
    monkeypatch.setattr(pipeline.common, 'process_kenburns', kenburns)
    ofrom, oto = synthetic.default_windows(48, 64)
    zoom = {'objectFrom': ofrom, 'objectTo': oto}
    depth = torch.full((1, 1, 48, 64), 200.0)
    depth[:, :, :24, :32] = 70.0

    def run(**settings):
        stub = _stub(pipeline, [], **settings)
        stub.objectCommon = {'tensorRawDepth': depth}
        stub.estimate = lambda tensorImage: None
        return stub(torch.zeros(1, 3, 48, 64), zoom, None)
    assert [f.shape for f in run()] == [(48, 64, 3)] * 2 and seen == [{'keep_on_device': False}]
    run(aperture=6)
    assert seen[1] == {'keep_on_device': False, 'lens': dof.Lens(200.0, 200.0, 6.0, 16)}                        # the centre of the end window, and it stays there
    run(aperture=2.5, focus=(5, 5), focus_to='60,40', width=32)
    assert seen[2] == {'keep_on_device': False, 'out_size': (32, 24), 'lens': dof.Lens(70.0, 200.0, 2.5, 16)}
    monkeypatch.setenv('KBE_APERTURE', '3')
    monkeypatch.setenv('KBE_FOCUS_TO', '5,5')
    run()
    assert seen[3] == {'keep_on_device': False, 'lens': dof.Lens(200.0, 70.0, 3.0, 16)}


def test_process_kenburns_and_render_frames_take_a_lens():
    from ken_burns_effect_amd import common, sharding
    assert inspect.signature(common.render_frames).parameters['lens'].default is None
    assert inspect.signature(common.process_kenburns).parameters['lens'].default is None
    with open(sharding.__file__) as f:
        assert 'lens' not in f.read()                                       # (the sharded path is out of scope: it does not take the argument)
    with pytest.raises(ValueError, match='needs crop'):
        common.render_frames([], {}, None, out_size=(4, 4), lens=(100.0, 50.0, 6.0))
    with pytest.raises(ValueError, match='^lens: aperture'):
        common.render_frames([], {}, None, lens=(100.0, 50.0, -6.0))
