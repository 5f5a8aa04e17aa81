"""The five tile filters on the GPU (kbe_area_reduce_u8, kbe_crop_area_u8, kbe_dof_u8, kbe_enlarge_u8, kbe_sharpen_u8) where their own test
modules do not reach: every alignment class of the tile store and of the row fetch -- one definition, csrc/kbe_rows.h, which every tile kernel
runs at its own loop shape, so each of the five is swept on its own --; sharpen's halo staging at every radius 1 .. 24, and enlarge at the
crops that fill its LDS row and its staged rectangle; of the first three the sides' limit of 65535 (enlarge's and sharpen's: their own
modules); and the radius of the blur as the device computes it, at its ties, at products that overflow and on subnormal depths.  Byte for byte
against the twins, or at the sides' limit against references that work there (tests/filter_sweep_cases.py; what they rest on:
tests/test_filter_sweeps.py), every buffer from guarded.Guard on both poisons."""
import numpy as np
import pytest
import torch

import dof_cases as dc
import enlarge_gpu as ng
import filter_gpu as fg
import filter_sweep_cases as fc
import sharpen_gpu as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def entries():
    """entry -> (its module, its raw call)"""
    from ken_burns_effect_amd import area, crop_area, dof, enlarge, sharpen
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    for module in (area, crop_area, dof, enlarge, sharpen):
        module.load()
    return {'area': (area, fg.run_area), 'crop_area': (crop_area, fg.run_crop_area), 'dof': (dof, fg.run_dof), 'enlarge': (enlarge, ng.run_enlarge),
            'sharpen': (sharpen, sg.run_sharpen)}


def assert_bytes(entries, entry, args, want, poison, **kw):
    """One call on guarded buffers full of the poison, every allocation on a multiple of 512 and the buffers their shifts off it: the expected
    bytes, the rows' padding unwritten, the bands intact (the raw call checks them)."""
    module, run = entries[entry]
    rc, got = run(module, *args, poison=poison, aligned=True, **kw)
    n, h, w, _ = want.shape
    assert rc == 0
    assert np.array_equal(got[:, :, :3 * w].reshape(n, h, w, 3), want), (entry, w, h, poison, kw)
    assert (got[:, :, 3 * w:] == poison).all(), (entry, w, h, poison, kw)


# -- 1. the alignment classes ------------------------------------------------------------------------
@pytest.mark.parametrize('poison', fg.POISONS, ids=hex)
@pytest.mark.parametrize('entry, variant', fc.STORE_SWEEPS, ids=str)
def test_every_lead_at_every_tile_width(entries, entry, variant, poison):
    """16 output rows an odd number of bytes apart -- every address mod 16 -- at every width 1 .. 64 of a single tile, and with a second and a
    third tile behind it: all 1024 classes of the store (tests/test_filter_sweeps.py), one call per width.  enlarge and sharpen have one
    width more that is 40 rows: tile rows beyond the first 16 and a second band."""
    for w in fc.store_widths(entry, variant):
        args, kw, want = fc.store_case(entry, variant, w)
        assert want.shape == (1, fc.store_rows(entry, w), w, 3) and 3 * w + kw['out_pad'] == fc.store_stride(w)
        assert_bytes(entries, entry, args, want, poison, **kw)


@pytest.mark.parametrize('poison', fg.POISONS, ids=hex)
@pytest.mark.parametrize('entry, variant', fc.FETCH_SWEEPS, ids=str)
def test_every_shift_at_every_length(entries, entry, variant, poison):
    """Source rows an odd number of bytes apart, the source 0, 1, 2 and 3 bytes off its allocation, four consecutive widths: all 16 classes of
    the aligned-dword fetch (tests/test_filter_sweeps.py)."""
    for W in fc.FETCH_WIDTHS[entry]:
        args, kw, want = fc.fetch_case(entry, variant, W)
        for src_shift in fc.SRC_SHIFTS:
            assert_bytes(entries, entry, args, want, poison, src_shift=src_shift, **kw)


# -- 1b. the code around the fetch that only sharpen and only enlarge have ---------------------------------
@pytest.mark.parametrize('R', fc.SHARPEN_RADII)
def test_sharpen_at_every_radius(entries, R):
    """Every R in 1 .. 24 -- each lays out the kernel's LDS its own way -- on frames where a staged row lies at every shift behind a left halo
    beyond the frame (3 R bytes rounded up to a dword), in front of a right halo that lies beyond it by all R pixels and by fewer, between
    both, and with neither; from R = 8 on with fewer rows than R (tests/test_filter_sweeps.py).  At R = 3 also with taps that do not fall
    with the distance."""
    for frame in fc.sharpen_radius_frames(R):
        for taps in (None, fc.ODD_TAPS) if R == len(fc.ODD_TAPS) - 1 else (None,):
            args, kw, want = fc.sharpen_radius_case(R, frame, taps)
            for poison in fg.POISONS:
                assert_bytes(entries, 'sharpen', args, want, poison, **kw)


@pytest.mark.parametrize('poison', fg.POISONS, ids=hex)
@pytest.mark.parametrize('i', range(len(fc.FULL_ROWS)), ids=['half', 'whole'])
def test_enlarge_at_a_full_raw_row(entries, i, poison):
    """190 x 46 from a crop 189 x 45: the middle tile stages 68 raw pixels at a shift of 3 -- all 52 dwords of an LDS row -- in 20 rows where
    the crop starts on half pixels, and 67 pixels of 19 rows, read by the pass along the rows itself, where it starts on whole pixels; the
    first and the last tile's span is cut by the clamp at the patch's border (tests/test_filter_sweeps.py).  The source 0 .. 3 bytes off."""
    args, kw, want = fc.full_row_case(i)
    for src_shift in fc.SRC_SHIFTS:
        assert_bytes(entries, 'enlarge', args, want, poison, src_shift=src_shift, **kw)


# -- 2. the sides' limit -------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', fg.POISONS, ids=hex)
@pytest.mark.parametrize('name', fc.LIMITS)
def test_area_at_the_sides_limit(entries, name, poison):
    """65535 x 2 and 2 x 65535 to themselves, to one pixel less, to just over half, to a ratio that is no integer and to one pixel: 1024 tiles
    across or 16384 down, span_end within 0.002 % of 2^32.  The expected bytes are the prefix sums'."""
    frame = fc.limit_frame(name)
    for w, h in fc.area_limit_targets(name):
        assert_bytes(entries, 'area', (frame, w, h), fc.exact_reduce(frame, w, h), poison, out_pad=1)


@pytest.mark.parametrize('poison', fg.POISONS, ids=hex)
@pytest.mark.parametrize('name', fc.LIMITS)
def test_crop_area_at_the_sides_limit(entries, name, poison):
    """Crops of those frames that start on a half pixel along the long side, on whole pixels, and that are the frame's own sides, each to the
    patch itself, to just over half of it and to one pixel."""
    frame = fc.limit_frame(name)
    for crop, size in fc.crop_limit_cases(name):
        assert_bytes(entries, 'crop_area', (frame, crop, size), fc.exact_crop_reduce(frame, crop, size), poison, out_pad=1)


@pytest.mark.parametrize('poison', fg.POISONS, ids=hex)
@pytest.mark.parametrize('name', fc.LIMITS)
def test_dof_at_the_sides_limit(entries, name, poison):
    """dof_cases' depths at 65535 x 2 and 2 x 65535, R = 16: the header's bytes (the twin's: tests/test_filter_sweeps.py)."""
    args = (fc.limit_frame(name), fc.limit_depth(name), dc.focus_of(1), dc.APERTURE, 16)
    assert_bytes(entries, 'dof', args, fc.limit_blur(name), poison, out_pad=1)


# -- 3. the radius as the device computes it -------------------------------------------------------------
@pytest.mark.parametrize('name', fc.RADIUS_ORDER)
def test_the_marks_spread_by_the_radius_of_the_definition(entries, name):
    """A black frame two tiles each way with radius 0 and three white marks in front of it whose depths are under test -- at a tie, one ulp to
    either side of it, with the aperture one ulp below; where A t and (j - 0.5) z overflow; subnormal -- across the tiles' borders.  The twin
    and the header agree on the marks' radii, the twin's bytes would be others at a radius one off (filter_sweep_cases.radius_case), and the
    device's bytes are the twin's."""
    frame, depth, want = fc.radius_case(name)
    zf, A = fc.RADIUS_CASES[name][:2]
    for poison in fg.POISONS:
        assert_bytes(entries, 'dof', (frame, depth, [zf], A, 16), want, poison, out_pad=5, pad=2, z_pad=1)
