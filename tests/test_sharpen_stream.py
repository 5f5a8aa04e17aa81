"""The output sharpening (include/kbe_sharpen.h) without a GPU: csrc/kbe_sharpen_block.h executed serially under its sanitizers
(tests/sharpen_check.cpp) against the four formulas in __int128 and against the NumPy twin (tests/sharpen_cases.py); the taps of a sigma; the
twin's properties and its distance to a float64 unsharp mask and to Pillow's; the binding (sharpen.py) held to what
tests/test_header_bindings.py holds the older headers to; and the command line's --sharpen and Pipeline(sharpen=)."""
import ctypes
import importlib
import os
import re
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest
from PIL import Image, ImageFilter

import gif_cases as gc
import sharpen_cases as sc
import test_header_bindings as thb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY = (r': cases (\d+), bytes (\d+), bad (\d+), negative (\d+), bad floors (\d+), clamped low (\d+), clamped high (\d+), kept (\d+), row max (\d+), column max (\d+), '
         r'gain max (\d+)')
ROW_BOUND, COLUMN_BOUND, GAIN_BOUND = 255 * 32768 + 64, 65280 * 32768 + 16384, 1024 * 65280 + 32768
ids = lambda v: v if isinstance(v, str) else 'R%d' % v if isinstance(v, int) else '%dx%d' % v                     # noqa: E731


# -- the definition ---------------------------------------------------------------------------
def test_the_header_against_the_formulas_in_int128():
    """sharpen_check.cpp builds under -fsanitize=signed-integer-overflow,address, and sharpen_pixel of csrc/kbe_sharpen_block.h equals the four
    formulas evaluated by brute force in __int128 for every R in 1..24: 24 radii x 4 sizes x 3 rounds; a floor is a floor for a negative
    amount * d too (thousands of them), both clamps and the threshold are met."""
    cases, count, bad, negative, bad_floors, low, high, kept, *_ = (int(v) for v in re.search('brute' + TALLY, sc.ask('brute')).groups())
    assert cases == 24 * 4 * 3 and count == 24 * 3 * 3 * (1 + 15 + 21 + 72) and bad == 0 and bad_floors == 0
    assert negative > 1000 and low > 0 and high > 0 and kept > 0


def test_the_32_bit_bounds_worst_cases_end_clean_under_the_sanitizer():
    """All-255 and all-0 frames and a 0 / 255 checkerboard at amount 1024 and 1, every R, all the weight on the centre tap, on the outermost
    pair and spread evenly: no signed overflow (the program would have aborted), the formulas' bytes, and the largest sums seen ARE the
    bounds the header states -- 255 * 32768 + 64 < 2^23, 65280 * 32768 + 16384 < 2^31 and 1024 * 65280 + 32768 < 2^27."""
    cases, count, bad, negative, bad_floors, low, high, kept, row, column, gain = (int(v) for v in re.search('limits' + TALLY, sc.ask('limits')).groups())
    assert cases == 24 * 3 * 3 * 4 and bad == 0 and bad_floors == 0 and negative > 0 and low > 0 and high > 0
    assert (row, column, gain) == (ROW_BOUND, COLUMN_BOUND, GAIN_BOUND) and row < 2 ** 23 and column < 2 ** 31 and gain < 2 ** 27
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'kbe_sharpen_block.h')) as f:
        text = f.read()
    assert '65280 * 32768 + 16384 = 2139111424 < 2^31' in text and '1024 * 65280 +' in text and '< 2^27' in text


@pytest.mark.parametrize('frame, R', sc.EVERY, ids=ids)
def test_the_header_is_the_twin(frame, R):
    """sharpen_pixel of csrc/kbe_sharpen_block.h on the GPU suite's frames, rows padded: the NumPy twin byte for byte."""
    W, H = frame
    assert np.array_equal(sc.header_sharpen(sc.frames(W, H), sc.taps_at(R), pad=5), sc.twin_of(W, H, R))
    if R == 2:
        for amount in sc.AMOUNTS:
            for threshold in sc.THRESHOLDS:
                assert np.array_equal(sc.header_sharpen(sc.frames(W, H), sc.taps_at(R), amount, threshold, pad=1), sc.twin_of(W, H, R, amount, threshold)), (amount, threshold)


def test_the_header_is_the_twin_on_thin_and_wide_frames():
    for W, H in sc.THIN:
        for R in (1, 24):
            assert np.array_equal(sc.header_sharpen(sc.thin(W, H), sc.taps_at(R), 1024), sc.twin_sharpen(sc.thin(W, H), sc.taps_at(R), 1024)), (W, H, R)
    assert np.array_equal(sc.header_sharpen(sc.wide(), sc.taps_at(7), 512, pad=3), sc.twin_sharpen(sc.wide(), sc.taps_at(7), 512))


# -- the taps ----------------------------------------------------------------------------------
def test_the_taps_of_a_sigma():
    """Every sigma 0.30, 0.31 .. 8.00: the sum is 32768, the taps do not increase with k and fit 16 bits, R = min(24, max(1, ceil(3 sigma))),
    and sharpen.taps_for is the twin's."""
    from ken_burns_effect_amd import sharpen
    for hundredths in range(30, 801):
        sigma = hundredths / 100.0
        w = sharpen.taps_for(sigma)
        assert w == sc.taps_of(sigma) and all(isinstance(v, int) for v in w)
        assert w[0] + 2 * sum(w[1:]) == sc.ONE == sharpen.ONE and all(a >= b for a, b in zip(w, w[1:])) and 0 <= w[-1] and w[0] < 65536, sigma
        assert len(w) - 1 == sc.radius_of(sigma) == min(24, max(1, int(np.ceil(3 * sigma))))
    assert sharpen.taps_for(0.3) == (32516, 126) and len(sharpen.taps_for(1.0)) == 4 and len(sharpen.taps_for(8)) == 25 == len(sharpen.taps_for(7.7))
    assert [len(sc.taps_at(R)) - 1 for R in sc.RADII] == list(sc.RADII)
    for sigma in (0.29, 8.01, 0, -1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r'sharpen\.taps_for: sigma'):
            sharpen.taps_for(sigma)


# -- properties of the twin --------------------------------------------------------------------
def test_constant_frames_and_1x1_frames_are_unchanged():
    for value in (0, 1, 137, 254, 255):
        for (W, H), R in sc.EVERY[:4] + [((1, 1), 1), ((1, 1), 24)]:
            frame = np.full((1, H, W, 3), value, np.uint8)
            assert (sc.twin_sharpen(frame, sc.taps_at(R), 1024) == value).all()
    assert (sc.header_sharpen(np.full((1, 9, 7, 3), 201, np.uint8), sc.taps_at(24), 1024) == 201).all()
    for R in sc.RADII:
        assert np.array_equal(sc.twin_sharpen(sc.thin(1, 1), sc.taps_at(R), 1024), sc.thin(1, 1))
        assert np.array_equal(sc.header_sharpen(sc.thin(1, 1), sc.taps_at(R), 1024), sc.thin(1, 1))


def test_amount_and_threshold_behave_as_defined():
    W, H = sc.FRAMES[0]
    frame, taps = sc.frames(W, H), sc.taps_at(2)
    v = frame.astype(np.int64)
    d = 256 * v - sc.twin_blur(frame, taps)
    assert np.abs(d).max() < 255 * 256 and (d < 0).any() and (d > 0).any()
    # threshold 255: no difference reaches it, the frame is its own output; threshold 0: every byte goes through the gain
    assert np.array_equal(sc.twin_sharpen(frame, taps, 1024, 255), frame)
    assert np.array_equal(sc.twin_sharpen(frame, taps, 256, 0), np.clip(v + ((256 * d + 32768) >> 16), 0, 255))
    # threshold 3: exactly the bytes whose difference is under 3 counts keep their value
    some = sc.twin_sharpen(frame, taps, 1024, 3)
    small = np.abs(d) < 3 * 256
    assert small.any() and (~small).any() and np.array_equal(some[small], frame[small]) and np.array_equal(some[~small], sc.twin_sharpen(frame, taps, 1024, 0)[~small])
    # amount 1 moves a byte by at most one count; a larger amount moves every byte at least as far, the same way
    one, full, four = (sc.twin_sharpen(frame, taps, amount).astype(np.int64) for amount in (1, 256, 1024))
    assert np.abs(one - v).max() <= 1 and (np.abs(four - v) >= np.abs(full - v)).all() and ((four - v) * (full - v) >= 0).all() and (four != full).any()
    # the channels are independent and are not swapped
    swapped = sc.twin_sharpen(np.ascontiguousarray(frame[..., ::-1]), taps, 700, 1)
    assert np.array_equal(swapped[..., ::-1], sc.twin_sharpen(frame, taps, 700, 1))
    # a frame's bytes do not depend on its neighbours
    five = sc.frames(W, H, 5)
    assert np.array_equal(sc.twin_sharpen(five, taps)[3], sc.twin_sharpen(five[3], taps))


FLOAT_CASES = [((37, 50), 0.3, 1.0), ((64, 48), 0.6, 4.0), ((160, 128), 1.0, 1.0), ((160, 128), 1.5, 1.5), ((160, 128), 2.3, 2.0), ((64, 48), 8.0, 4.0), ((37, 50), 8.0, 0.5)]
MEASURED = 1                                                           # the largest difference over FLOAT_CASES, in counts: see the docstring below


def test_the_distance_to_a_float64_unsharp_mask():
    """A condition on the twin, not on the device.  The same mask in float64 -- exact Gaussian weights over the same radius, the edge
    replicated, rounded half up and clamped once at the end -- against the twin: the taps' 15 bits and the two 8.8 roundings of the blur
    move the result by less than a count before the final rounding, which can then fall the other way.  Measured over the cases below: at
    most 1 count (on 0.02 to 0.80 % of the bytes, the most at amount 4); held to that measured maximum plus one, the margin one rounding
    of the final shift."""
    worst = 0
    for (W, H), sigma, amount in FLOAT_CASES:
        frame = sc.frames(W, H)
        mine = sc.twin_sharpen(frame, sc.taps_of(sigma), int(np.floor(256 * amount + 0.5))).astype(np.int64)
        exact = np.clip(np.floor(sc.float_sharpen(frame, sigma, amount) + 0.5), 0, 255).astype(np.int64)
        apart = np.abs(mine - exact)
        print('%dx%d sigma %g amount %g: at most %d counts, %.2f %% of the bytes' % (W, H, sigma, amount, apart.max(), 100.0 * (apart != 0).mean()))
        worst = max(worst, int(apart.max()))
    assert worst <= MEASURED + 1
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        assert 'at most %d count' % MEASURED in f.read()


def test_pillows_unsharp_mask_as_a_neighbour():
    """Measured and reported, not matched: Pillow's ImageFilter.UnsharpMask blurs with a box approximation of the Gaussian (three box passes
    of an extended-box radius) and truncates where the twin rounds, so the two are neighbours and not twins.  The one thing asserted is that
    both sharpen: each lies farther from the frame than from the other, in the mean."""
    for (W, H), sigma, percent in (((160, 128), 1.0, 100), ((160, 128), 2.3, 150), ((64, 48), 1.5, 200)):
        frame = sc.frames(W, H, 1)[0]
        mine = sc.twin_sharpen(frame, sc.taps_of(sigma), int(np.floor(256 * percent / 100.0 + 0.5))).astype(np.int64)
        theirs = np.asarray(Image.fromarray(frame).filter(ImageFilter.UnsharpMask(radius=sigma, percent=percent, threshold=0))).astype(np.int64)
        apart, moved = np.abs(mine - theirs), np.abs(mine - frame.astype(np.int64))
        print('%dx%d sigma %g percent %d: Pillow differs by at most %d counts, %.2f in the mean; the mask moves a byte by %.2f in the mean' % (
            W, H, sigma, percent, apart.max(), apart.mean(), moved.mean()))
        assert apart.mean() < moved.mean()


# -- the binding -------------------------------------------------------------------------------
p, i = c_void_p, c_int
TAPS = (ctypes.c_uint16 * 2)(32516, 126)
NULL_CALL = (None, 1, 4, 4, 12, None, 12, TAPS, 1, 256, 0, None)
OLDER = [('kbe.h', '#define KBE_ABI_VERSION 13\n'), ('kbe_gif.h', '#define KBE_GIF_ABI_VERSION 1\n'), ('kbe_area.h', '#define KBE_AREA_ABI_VERSION 1\n'),
         ('kbe_crop_area.h', '#define KBE_CROP_AREA_ABI_VERSION 1\n'), ('kbe_dof.h', '#define KBE_DOF_ABI_VERSION 1\n'), ('kbe_shutter.h', '#define KBE_SHUTTER_ABI_VERSION 1\n'),
         ('kbe_yuv.h', '#define KBE_YUV_ABI_VERSION 1\n'), ('kbe_transition.h', '#define KBE_TRANSITION_ABI_VERSION 1\n'), ('kbe_overlay.h', '#define KBE_OVERLAY_ABI_VERSION 1\n'),
         ('kbe_grade.h', '#define KBE_GRADE_ABI_VERSION 1\n'), ('kbe_enlarge.h', '#define KBE_ENLARGE_ABI_VERSION 1\n')]
SHARPEN = thb.Binding(
    'sharpen', 'kbe_sharpen',
    # frames, n, W, H, stride; out, out stride; taps, radius, amount, threshold; stream
    {'kbe_sharpen_abi_version': (c_int, []), 'kbe_sharpen_u8': (c_int, [p, i, i, i, i, p, i, p, i, i, i, p])},
    'kbe_sharpen_abi_version', ['#define KBE_SHARPEN_ABI_VERSION 1\n'], ['KBE_SHARPEN_BGR'], {'ABI_VERSION': 1, 'MAX_SIDE': 65535, 'MAX_RADIUS': 24, 'ONE': 32768, 'MAX_AMOUNT': 1024},
    OLDER,
    ('kbe_sharpen_u8', NULL_CALL, 'kbe_sharpen_u8: null frames_u8'),
    ('kbe_sharpen_u8', None, lambda frames: ((frames, 1.0, 4, 4, 12, frames, 12, TAPS, 1, 256, 0, None), (frames, 1, 4, 4, 12, frames, 12, TAPS, 1, 256, c_size_t(0), None),
                                             (frames, 1, 4, 4, 12, frames, 12, TAPS, 1, 256, 0))),
    [('kbe_sharpen_abi_version', 0, (1,)), ('kbe_sharpen_u8', 12, NULL_CALL + (0,)), ('kbe_sharpen_u8', 12, NULL_CALL[:-1])],
    ['kbe_enlarge_u8', 'kbe_crop_area_u8', 'kbe_area_reduce_u8', 'kbe_grade_u8', 'kbe_dof_u8', 'kbe_gif_bound', 'kbe_png_bound'],
    ('kbe_sharpen_u8', lambda at: ((c_void_p * 2)(at, at + 1024), 2, 16, 17, 48, (c_void_p * 2)(at + 4096, at + 6144), 48, TAPS, 1, 1025, 0, None),
     'kbe_sharpen_u8 failed (-1): kbe_sharpen_u8: amount outside 1..1024'),
    ['kbe_sharpen_u8'], set())
# what the other headers' modules declare: the lists this header must leave as they are
OTHERS = {'gif': list(thb.GIF.protos), 'area': list(thb.AREA.protos), 'crop_area': ['kbe_crop_area_abi_version', 'kbe_crop_area_u8'], 'dof': ['kbe_dof_abi_version', 'kbe_dof_u8'],
          'shutter': ['kbe_shutter_abi_version', 'kbe_shutter_mean_u8'], 'yuv': ['kbe_yuv_abi_version', 'kbe_yuv420_bytes', 'kbe_yuv420_u8'],
          'transition': ['kbe_transition_abi_version', 'kbe_transition_u8'], 'overlay': ['kbe_overlay_abi_version', 'kbe_overlay_u8'], 'grade': ['kbe_grade_abi_version', 'kbe_grade_u8'],
          'enlarge': ['kbe_enlarge_abi_version', 'kbe_enlarge_u8']}


def test_the_header_parses_to_exactly_its_two_entries():
    thb.test_the_header_parses_to_exactly_its_entries(SHARPEN)
    from ken_burns_effect_amd import sharpen
    assert list(sharpen.prototypes()) == ['kbe_sharpen_abi_version', 'kbe_sharpen_u8']


def test_the_library_exports_them_beside_the_others():
    thb.test_the_library_exports_them_with_the_headers_types(SHARPEN)
    from ken_burns_effect_amd import _native, sharpen
    lib = sharpen.load()
    assert lib is _native.load() and lib.kbe_sharpen_abi_version() == 1 == sharpen.ABI_VERSION
    for name, entries in OTHERS.items():
        module = importlib.import_module('ken_burns_effect_amd.' + name)
        assert module.load() is lib and getattr(lib, entries[0])() == 1


def test_the_older_headers_and_their_bindings_are_what_they_were():
    from ken_burns_effect_amd import _native, sharpen
    b = SHARPEN
    sharpen.load()
    assert len(_native.SYMBOLS) == 48 and not any(name.startswith(b.prefix) for name in _native.SYMBOLS)
    for header, number in b.older:
        with open(os.path.join(ROOT, 'include', header)) as f:
            text = f.read()
        assert b.prefix not in text and b.prefix.upper() not in text and number in text
    assert _native.load().kbe_abi_version() == 13
    for name, entries in OTHERS.items():
        other = importlib.import_module('ken_burns_effect_amd.' + name)
        assert list(other.prototypes()) == entries and other.ABI_VERSION == 1
    # sharpen.py is the only module of the package whose text names the header's prefix, and it names no entry of another header
    package = os.path.dirname(sharpen.__file__)
    naming = [name for name in sorted(os.listdir(package)) if name.endswith('.py') and b.prefix in open(os.path.join(package, name)).read()]
    assert naming == ['sharpen.py']
    with open(sharpen.__file__) as f:
        text = f.read()
    foreign = set(_native.SYMBOLS) | {entry for entries in OTHERS.values() for entry in entries}
    assert not [entry for entry in sorted(foreign) if entry in text]
    name, args, text = b.null_call
    assert sharpen._raw(name, *args) == -1 and _native.load().kbe_last_error().decode() == text


def test_ctypes_refuses_a_wrong_call_before_it_is_made():
    thb.test_ctypes_refuses_a_wrong_call_before_it_is_made(SHARPEN)


def test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused():
    thb.test_a_surplus_or_missing_argument_and_another_headers_entry_are_refused(SHARPEN)


def test_call_reports_a_refusal_with_the_librarys_text():
    thb.test_call_reports_a_refusal_with_the_librarys_text(SHARPEN)


def test_every_call_site_passes_the_headers_number_of_arguments():
    thb.test_every_call_site_passes_the_headers_number_of_arguments(SHARPEN)


def test_the_makefile_builds_the_source():
    with open(os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc', 'Makefile')) as f:
        text = f.read()
    assert ' kbe_sharpen.hip' in text and ' kbe_sharpen_block.h' in text and '../../include/kbe_sharpen.h' in text


SUM = 'taps[0] + 2 (taps[1] + .. + taps[radius]) is not 32768'
REFUSED = {'null frames': (dict(frames_u8=None), 'null frames_u8'), 'null out': (dict(out_u8=None), 'null out_u8'), 'null taps': (dict(taps=None), 'null taps'),
           'n = 0': (dict(n_frames=0), 'n_frames < 1'), 'W = 0': (dict(W=0), 'W or H outside 1..65535'), 'H = 65536': (dict(H=65536), 'W or H outside 1..65535'),
           'stride': (dict(stride_bytes=47), 'stride_bytes < 3 W'), 'out stride': (dict(out_stride_bytes=47), 'out_stride_bytes < 3 W'),
           'radius = 0': (dict(radius=0), 'radius outside 1..24'), 'radius = 25': (dict(radius=25), 'radius outside 1..24'),
           'taps short': (dict(taps=(ctypes.c_uint16 * 2)(32516, 125)), SUM), 'taps long': (dict(taps=(ctypes.c_uint16 * 3)(32516, 126, 1), radius=2), SUM),
           'amount = 0': (dict(amount=0), 'amount outside 1..1024'), 'amount = 1025': (dict(amount=1025), 'amount outside 1..1024'),
           'threshold = -1': (dict(threshold=-1), 'threshold outside 0..255'), 'threshold = 256': (dict(threshold=256), 'threshold outside 0..255'),
           'null frame 1': (dict(frames_u8=1), 'null element of frames_u8'), 'null output 1': (dict(out_u8=1), 'null element of out_u8')}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_the_refusal_texts(what):
    """Every argument is refused before anything is enqueued, on host memory no kernel could touch, and the text names the entry and the argument."""
    from ken_burns_effect_amd import _native, sharpen
    memory = (ctypes.c_uint64 * 1024)()
    at = ctypes.addressof(memory)
    args = dict(frames_u8=(c_void_p * 2)(at, at + 1024), n_frames=2, W=16, H=17, stride_bytes=48, out_u8=(c_void_p * 2)(at + 4096, at + 6144), out_stride_bytes=50, taps=TAPS, radius=1,
                amount=256, threshold=0, stream=None)
    change, text = REFUSED[what]
    for key, value in change.items():
        if key in ('frames_u8', 'out_u8') and value == 1:
            args[key][1] = None
        else:
            args[key] = value
    assert sharpen._raw('kbe_sharpen_u8', *args.values()) == -1
    assert _native.load().kbe_last_error().decode() == 'kbe_sharpen_u8: ' + text
    assert not any(memory)


def test_apply_sharpen_refuses_what_is_no_tensor_on_the_gpu():
    import torch
    from ken_burns_effect_amd import _native, sharpen
    with pytest.raises(_native.KbeError, match=r'sharpen\.apply_sharpen takes a contiguous uint8 \[n,H,W,3\] tensor on the GPU'):
        sharpen.apply_sharpen(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), sharpen.request('1', environment=False))


# -- the option ----------------------------------------------------------------------------------
GOOD = {'1': (256, 1.0, 0), '1,1.5': (256, 1.5, 0), '0.5,2,3': (128, 2.0, 3), '4,8,255': (1024, 8.0, 255), '0.002,0.3': (1, 0.3, 0), ' 1.5 , 0.6 , 1 ': (384, 0.6, 1)}
BAD = [('x', r'^--sharpen x: AMOUNT\[,SIGMA\[,THRESHOLD\]\]: two numbers and a whole number$'), ('1,,3', r'^--sharpen 1,,3: AMOUNT\[,SIGMA'), ('1,1,1.5', r'^--sharpen 1,1,1\.5: AMOUNT\[,SIGMA'),
       ('nan', r'^--sharpen nan: AMOUNT\[,SIGMA'), ('0', r'^--sharpen 0: AMOUNT 0: above 0 and at most 4$'), ('4.01', r'^--sharpen 4\.01: AMOUNT 4\.01: above 0 and at most 4$'),
       ('-1', r'^--sharpen -1: AMOUNT -1: above 0 and at most 4$'), ('0.001', r'^--sharpen 0\.001: AMOUNT 0\.001: above 0 and at most 4$'), ('inf', r'^--sharpen inf: AMOUNT inf: above 0 and at most 4$'),
       ('1,0.29', r'^--sharpen 1,0\.29: SIGMA 0\.29: 0\.3\.\.8$'), ('1,8.5', r'^--sharpen 1,8\.5: SIGMA 8\.5: 0\.3\.\.8$'), ('1,1,256', r'^--sharpen 1,1,256: THRESHOLD 256: a whole number 0\.\.255$'),
       ('1,1,-1', r'^--sharpen 1,1,-1: THRESHOLD -1: a whole number 0\.\.255$'), ('1,2,3,4', r'^--sharpen 1,2,3,4: 4 fields: AMOUNT\[,SIGMA\[,THRESHOLD\]\], three at most$')]


def test_the_request(monkeypatch):
    from ken_burns_effect_amd import sharpen
    monkeypatch.delenv('KBE_SHARPEN', raising=False)
    assert sharpen.request() is None and sharpen.request(None) is None
    for text, (amount, sigma, threshold) in GOOD.items():
        got = sharpen.request(text)
        assert got == {'amount': amount, 'sigma': sigma, 'threshold': threshold, 'taps': sc.taps_of(sigma), 'radius': sc.radius_of(sigma)}, text
    assert sharpen.request((1.5, 0.6, 1)) == sharpen.request('1.5,0.6,1') == sharpen.request([1.5, '0.6', '1']) and sharpen.request(2) == sharpen.request('2') == sharpen.request((2,))
    for text, match in BAD:
        with pytest.raises(ValueError, match=match):
            sharpen.request(text)
    for value in ((1, 2, 3, 4), (1, 1, 1.5), (True,), (1, None), (1, 1, True)):
        with pytest.raises(ValueError, match=r'^--sharpen '):
            sharpen.request(value)
    monkeypatch.setenv('KBE_SHARPEN', '0.5,2,3')
    assert sharpen.request() == sharpen.request('0.5,2,3') and sharpen.request('1')['amount'] == 256 and sharpen.request(environment=False) is None
    monkeypatch.setenv('KBE_SHARPEN', '9')
    with pytest.raises(ValueError, match=r'^--sharpen 9: AMOUNT 9: above 0 and at most 4$'):
        sharpen.request()


def test_the_command_line_takes_the_option(monkeypatch):
    from ken_burns_effect_amd import kbe, slideshow
    monkeypatch.delenv('KBE_SHARPEN', raising=False)
    cfg = kbe.parse([])[0]
    assert cfg['sharpen'] is None and cfg['sharpened'] is None
    cfg = kbe.parse(['--sharpen', '1,1.5', '--width', '1920', '--enlarge'])[0]
    assert cfg['sharpen'] == '1,1.5' and cfg['sharpened']['amount'] == 256 and cfg['sharpened']['radius'] == 5
    assert 'sharpen=' in kbe.LONG_OPTIONS and '[--sharpen AMOUNT[,SIGMA[,THRESHOLD]]]' in kbe.__doc__ and 'KBE_SHARPEN' in kbe.__doc__
    assert 'sharpen=' in slideshow.LONG_OPTIONS and '[--sharpen AMOUNT[,SIGMA[,THRESHOLD]]]' in slideshow.__doc__
    assert slideshow.parse(['--in', 'a.png', '--sharpen', '0.5,2,3'])['sharpened'] == kbe.parse(['--sharpen', '0.5,2,3'])[0]['sharpened']
    for text, match in BAD:
        with pytest.raises(SystemExit, match=match):
            kbe.parse(['--sharpen', text])
        with pytest.raises(SystemExit, match=match):
            slideshow.parse(['--in', 'a.png', '--in', 'b.png', '--sharpen', text])


def _stub(P, calls, sharpen=None):
    import torch

    class Stub(P.Pipeline):
        def __init__(self):
            self.output_frames, self.dolly, self.steps, self.objectCommon, self.moduleInpaint, self.device = False, False, 2, {}, None, torch.device('cpu')
            self.sharpen = sharpen

        def estimate(self, tensorImage):
            calls.append('estimate')
            raise AssertionError('a network ran')
    return Stub()


def test_the_refusals_come_before_a_network_runs(tmp_path, monkeypatch):
    import torch
    from ken_burns_effect_amd import kbe, pipeline, slideshow
    for name in ('KBE_WIDTH', 'KBE_ENLARGE', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_SHARPEN'):
        monkeypatch.delenv(name, raising=False)
    calls = []
    monkeypatch.setattr(pipeline.common, 'process_kenburns', lambda *a, **k: calls.append('render'))
    image = torch.zeros(1, 3, 48, 64)
    zoom = kbe.windows_for(64, 48, slideshow.NO_WINDOW, False)
    out = str(tmp_path / 'out')
    for text, match in BAD:
        with pytest.raises(ValueError, match=match):
            _stub(pipeline, calls, text)(image, zoom, out)
        with pytest.raises(ValueError, match=match):
            _stub(pipeline, calls, text).render(image, zoom)
    with pytest.raises(ValueError, match=r'^--sharpen 1,2,3,4: 4 fields'):
        _stub(pipeline, calls, (1, 2, 3, 4))(image, zoom, out)
    monkeypatch.setenv('KBE_SHARPEN', '1,9')
    with pytest.raises(ValueError, match=r'^--sharpen 1,9: SIGMA 9: 0\.3\.\.8$'):
        _stub(pipeline, calls)(image, zoom, None)
    with pytest.raises(ValueError, match=r'^--sharpen 1,9: SIGMA 9: 0\.3\.\.8$'):
        slideshow.make([image, image], out, _stub(pipeline, calls), 'dissolve', 1)
    monkeypatch.delenv('KBE_SHARPEN')
    assert calls == [] and not (tmp_path / 'out').exists()
    assert pipeline.sharpen_of(_stub(pipeline, calls)) is None and pipeline.sharpen_of(_stub(pipeline, calls, '1'))['amount'] == 256
    frames = object()
    assert pipeline.with_sharpen(None, frames) is frames
    # the command lines: before Pipeline is built
    built = []
    monkeypatch.setattr(pipeline.Pipeline, '__init__', lambda self, *a, **k: built.append(k))
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(48, 64, 1)).save(path)
    grad = torch.is_grad_enabled()
    try:                                                                   # (main switches autograd off for its process)
        with pytest.raises(SystemExit, match=r'^--sharpen 5: AMOUNT 5: above 0 and at most 4$'):
            kbe.main(['--in', path, '--out', out, '--sharpen', '5'])
        with pytest.raises(SystemExit, match=r'^--sharpen 1,2,3,4: 4 fields'):
            slideshow.main(['--in', path, '--in', path, '--out', out, '--sharpen', '1,2,3,4'])
    finally:
        torch.set_grad_enabled(grad)
    assert built == [] and not (tmp_path / 'out').exists()


def test_the_keyword_reaches_the_pipeline_and_is_absent_without_the_option(tmp_path, monkeypatch):
    """kbe.main and slideshow.main pass sharpen= to Pipeline only where the option was given: without it the call is what it was."""
    import torch
    from ken_burns_effect_amd import kbe, pipeline, slideshow

    class Built(Exception):
        pass
    built = []

    def init(self, *a, **k):
        built.append(k)
        raise Built()
    monkeypatch.delenv('KBE_SHARPEN', raising=False)
    monkeypatch.setattr(pipeline.Pipeline, '__init__', init)
    path = str(tmp_path / 'in.png')
    Image.fromarray(gc.photo_like(48, 64, 1)).save(path)
    grad = torch.is_grad_enabled()
    try:
        for main, argv in ((kbe.main, ['--in', path]), (slideshow.main, ['--in', path, '--in', path])):
            with pytest.raises(Built):
                main(argv + ['--out', str(tmp_path / 'out')])
            with pytest.raises(Built):
                main(argv + ['--out', str(tmp_path / 'out'), '--sharpen', '1,1.5'])
    finally:
        torch.set_grad_enabled(grad)
    assert ['sharpen' in k for k in built] == [False, True, False, True] and built[1]['sharpen'] == '1,1.5' == built[3]['sharpen']
    with open(os.path.join(os.path.dirname(pipeline.__file__), 'sharding.py')) as f:
        assert 'sharpen' not in f.read()                                    # (the sharded path is out of scope: it does not learn the option)
    import inspect
    monkeypatch.undo()                                                      # (the real __init__ again)
    assert inspect.signature(pipeline.Pipeline.__init__).parameters['sharpen'].default is None
