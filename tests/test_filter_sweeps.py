"""What tests/test_filter_sweeps_gpu.py rests on, without a GPU (tests/filter_sweep_cases.py): the sweeps' parameters reach every alignment class
of the tile store and row fetch that the kernels share (csrc/kbe_rows.h), by the launch arithmetic alone -- and every class of sharpen's halo
staging at every radius, and enlarge's full LDS row --; that header itself, executed serially (tests/rows_check.cpp); the twins of the
enlargement and the sharpening equal their headers at the sweeps' shapes; the exact area reduction by prefix sums equals the headers and the
twins wherever both exist, the sides' limit among them; and every frame that makes a radius visible is sensitive to it."""
import re
import subprocess

import numpy as np
import pytest

import area_cases as ac
import crop_area_cases as cc
import dof_cases as dc
import enlarge_cases as ec
import filter_sweep_cases as fc
import sharpen_cases as sc
import twins


# -- the shared row fetch and piece store, as compiled ---------------------------------------------
def test_the_rows_header_is_the_bytes_themselves():
    """rows_check.cpp builds.  store_piece over rows of 1..80 bytes at every lead, into 0x5A between bands: every byte of the row written
    exactly once, nothing else changed, and every piece on the path the rule says -- counted here again from the rule: a piece whose 16
    bytes are all the row's goes as 16 bytes; of any other, a dword whose four bytes are all the row's as a dword, the rest as bytes.  The
    tile row at real addresses, the fetch arithmetic, realign<4, 6, 12> and the dwords' rule by brute force: no mismatch."""
    out = subprocess.run([twins.built('rows_check'), 'brute'], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout + out.stderr)[-1000:]
    m = re.search(r'brute: pieces (\d+), piece mismatches (\d+), whole pieces (\d+), dwords (\d+), bytes (\d+), tile rows (\d+), tile row mismatches (\d+), fetches (\d+), '
                  r'fetch mismatches (\d+), realign mismatches (\d+), dwords asked (\d+), dword rule mismatches (\d+)', out.stdout)
    pieces, piece_bad, whole, dwords, single, tile_rows, tile_bad, fetches, fetch_bad, realign_bad, asked, rule_bad = (int(v) for v in m.groups())
    want = {'pieces': 0, 'whole': 0, 'dwords': 0, 'bytes': 0}
    for n in range(1, 81):
        for lead in range(16):
            for at in range(0, lead + n, 16):
                mine = [lead <= at + i < lead + n for i in range(16)]
                want['pieces'] += 1
                if all(mine):
                    want['whole'] += 1
                    continue
                for d in range(4):
                    four = mine[4 * d:4 * d + 4]
                    want['dwords' if all(four) else 'bytes'] += 1 if all(four) else sum(four)
    assert want['whole'] > 0 and want['dwords'] > 0 and want['bytes'] > 0
    assert (pieces, whole, dwords, single) == (want['pieces'], want['whole'], want['dwords'], want['bytes'])
    assert (tile_rows, fetches) == (64 * 16, 40 * 4)
    assert asked == sum((n + 3 + 19 + 1) * 4 * (N + 1) for N in (4, 12) for n in range(1, 41))
    assert (piece_bad, tile_bad, fetch_bad, realign_bad, rule_bad) == (0, 0, 0, 0, 0)


# -- the classes -----------------------------------------------------------------------------------
@pytest.mark.parametrize('entry, variant', fc.STORE_SWEEPS, ids=str)
def test_the_store_sweep_reaches_every_lead_at_every_tile_width(entry, variant):
    """16 leads x 64 tile widths, given that an allocation starts on a multiple of 512 (16 is what matters): all 1024 for every sweep over all
    the widths; area's sweep at ratio 1 takes at least eight widths, each at every lead.  The widths of 16 rows alone reach them all: the
    taller ones of enlarge and sharpen are there for the tile rows, not for the leads."""
    found = fc.store_sweep_classes(entry, variant)
    widths = fc.store_widths(entry, variant)
    assert fc.STORE_ROWS == 16 and all(fc.store_rows(entry, w) == 16 for w in fc.STORE_WIDTHS + fc.COPY_WIDTHS)
    if (entry, variant) == ('area', 'copy'):
        assert len(widths) >= 8 and found == {(lead, min(w - ox0, 64)) for w in widths for ox0 in range(0, w, 64) for lead in range(16)}
    else:
        assert set(range(1, 65)) <= set(widths) and {65, 127, 128, 129} <= set(widths)
        assert found == fc.EVERY_STORE_CLASS and len(found) == 1024
    assert all(fc.store_stride(w) % 2 == 1 and fc.store_stride(w) > 3 * w for w in widths)           # odd, and with padding that must stay unwritten
    if entry in ('enlarge', 'sharpen'):
        assert set().union(*(fc.store_classes(w, 16, fc.store_stride(w)) for w in fc.STORE_WIDTHS)) == fc.EVERY_STORE_CLASS


def test_the_store_sweeps_of_enlarge_and_sharpen_take_every_route_and_every_tile_row():
    """enlarge: the crop that starts on whole pixels (the pass along the rows reads the staged raw rows) and on half pixels (it reads the
    patch), every case a true enlargement down the columns and from w = 3 on along the rows, and an output three bands down whose second band is whole: tile rows 0 .. 15 of a
    workgroup that is not the first.  sharpen: a radius of at most 2 and the largest, and an output of more than 32 rows, three tiles
    across: the store's second trip (tile rows 16 .. 31) and a second band, which is cut."""
    sweeps = set(fc.STORE_SWEEPS)
    assert {('enlarge', 'oo'), ('enlarge', 'ee')} <= sweeps and (cc.OFF['oo'][0] % 2, cc.OFF['oo'][1] % 2, cc.OFF['ee'][0] % 2, cc.OFF['ee'][1] % 2) == (1, 1, 0, 0)
    radii = sorted(v for e, v in sweeps if e == 'sharpen')
    assert len(radii) >= 2 and radii[0] <= 2 and radii[-1] == 24 == fc.MAX_RADIUS
    assert fc.TILE_Y['enlarge'] == 16 and fc.TILE_Y['sharpen'] == 32
    for variant in ('oo', 'ee'):
        for w in fc.store_widths('enlarge', variant):
            (frames, crop, size), _, want = fc.store_case('enlarge', variant, w)
            assert size == (w, fc.store_rows('enlarge', w)) and 1 <= crop[0] <= w and crop[1] < size[1] and (crop[0] < w or w <= 2)
            assert frames.shape[1:3] == (crop[1] + cc.OFF[variant][1], crop[0] + cc.OFF[variant][0]) and want.shape == (1, size[1], w, 3)
    tall = {entry: max((fc.store_rows(entry, w), w) for w in fc.store_widths(entry, 'oo' if entry == 'enlarge' else 2)) for entry in ('enlarge', 'sharpen')}
    assert tall['enlarge'][0] >= 2 * 16 + 1 and tall['sharpen'][0] > 32 and all(2 * 64 < w <= 3 * 64 and h <= 48 for h, w in tall.values())
    for R in radii:
        for w in fc.store_widths('sharpen', R):
            (frames, taps, amount), _, want = fc.store_case('sharpen', R, w)
            assert len(taps) == R + 1 and frames.shape == want.shape == (1, fc.store_rows('sharpen', w), w, 3)
        assert (fc.store_case('sharpen', R, 64)[2] != fc.store_case('sharpen', R, 64)[0][0]).mean() > 0.2                # (the mask does something)


@pytest.mark.parametrize('entry, variant', fc.FETCH_SWEEPS, ids=str)
def test_the_fetch_sweep_reaches_every_shift_at_every_length(entry, variant):
    """4 shifts x 4 values of 3 len mod 4, the source 0, 1, 2 and 3 bytes off its allocation and its rows an odd number of bytes apart."""
    assert fc.SRC_SHIFTS == (0, 1, 2, 3) and all(fc.fetch_stride(W) % 2 == 1 for W in range(1, 500))
    found = fc.fetch_sweep_classes(entry, variant)
    assert found == fc.EVERY_FETCH_CLASS and len(found) == 16


def test_the_classes_of_a_known_call():
    """By hand.  20 pixels a row, rows 61 bytes apart, 2 bytes off: row 0 leads by 2, row 1 by 63 mod 16 = 15; 70 pixels: a tile of 64 and one
    of 6 with the same lead.  area 9 x 2 -> 3 x 1 at a stride of 29, 1 byte off: one strip of 9 pixels, rows at 1 and 30: shifts 1 and 2, 27 mod 4 = 3."""
    assert fc.store_classes(20, 2, 61, shift=2) == {(2, 20), (15, 20)}
    assert fc.store_classes(70, 1, 211) == {(0, 64), (0, 6)}
    assert fc.area_fetch_classes(9, 2, 3, 1, 29, 1) == {(1, 3), (2, 3)}
    # crop 8 x 2 of 12 x 2 starts at pixel 2, half a pixel on: 9 raw pixels (the second taps) from byte 6 of rows 0 and 1; dof: the whole row of 5
    assert fc.crop_area_fetch_classes(12, 2, (8, 2), (4, 1), 37, 0) == {(2, 3), (3, 3)}
    assert fc.dof_fetch_classes(5, 1, 16, 15, 3) == {(3, 3)}
    # sharpen 70 x 2 at R = 1, rows 211 bytes apart, 1 byte off.  The tile at 0 stages pixels 0 .. 64 (65: 195 mod 4 = 3) of the frame rows
    # clamp(-1 .. 2) = 0, 0, 1, 1 at 1 and 212: shifts 1 and 0, its left halo of 1 beyond the frame.  The tile at 64, 6 wide, stages pixels
    # 63 .. 69 (7: 21 mod 4 = 1) at 1 + 189 = 190 and 212 + 189 = 401: shifts 2 and 1, its right halo of 1 beyond the frame
    assert fc.sharpen_fetch_classes(70, 2, 1, 211, 1) == {(1, 3), (0, 3), (2, 1), (1, 1)}
    assert fc.sharpen_stage_classes(70, 2, 1, 211, 1) == {(1, 1, 'left'), (0, 1, 'left'), (2, 1, ('right', 1)), (1, 1, ('right', 1))}
    # ... 5 x 1 at R = 2, 3 bytes off: one tile, both halos of 2 beyond the frame, five staged rows that are all row 0
    assert fc.sharpen_stage_classes(5, 1, 2, 15, 3) == {(3, 2, ('both', 2))} and fc.sharpen_fetch_classes(5, 1, 2, 15, 3) == {(3, 3)}
    # enlarge: the crop 8 x 2 of 12 x 2 above to 16 x 2.  Along x the first target lies at i = floor(-8 / 32) = -1 and the last at
    # floor((31 * 8 - 16) / 32) = 7: the taps -2 .. 9 clamped are the whole patch, 8 pixels and the second taps' one more, 9 raw pixels
    # from pixel 2.  Along y the taps of 2 -> 2 are rows -1 .. 3 clamped, 0 and 1, and the third row the second taps ask for is not there
    assert fc.enlarge_fetch_classes(12, 2, (8, 2), (16, 2), 37, 0) == ({(2, 3), (3, 3)}, (9, 3), 2)
    assert fc.enlarge_cuts(8, 16, 64) == [(True, True)]


# -- sharpen's halo staging ------------------------------------------------------------------------------
@pytest.mark.parametrize('R', fc.SHARPEN_RADII)
def test_the_frames_of_a_radius_reach_every_halo_at_every_shift(R):
    """At every R in 1 .. 24, a staged row at every shift 0 .. 3 in a tile whose left halo lies beyond the frame, in one whose right halo
    does by fewer than R pixels and in one where it does by all R, in a tile with both beyond it (W < 64) and in one with neither.  At R = 1
    there is no count between 0 and R: that class does not exist.  Frames of fewer rows than R -- every staged row above and below the tile
    a border row -- are among them from R = 8 on at the latest."""
    assert fc.SHARPEN_RADII == tuple(range(1, 25))
    found, frames = fc.sharpen_radius_classes(R), fc.sharpen_radius_frames(R)
    assert {r for _, r, _ in found} == {R}
    for border in ['neither', 'left', ('right', R), ('both', R)]:
        assert {shift for shift, _, b in found if b == border} == {0, 1, 2, 3}, border
    part = {b[1] for _, _, b in found if b[0] == 'right' and 0 < b[1] < R}
    assert len(part) == (1 if R >= 2 else 0)
    for right in part:
        assert {shift for shift, _, b in found if b == ('right', right)} == {0, 1, 2, 3}
    assert all(W <= 3 * 64 and 4 <= H <= 48 and fc.fetch_stride(W) % 2 == 1 for W, H in frames) and any(W < 64 for W, _ in frames)
    if R >= 8:
        assert all(H < R for _, H in frames)
    # the slack between the left halo and the first fetched dword, (3 R + 3 & ~3) - 3 R, takes every value it can over the radii
    assert {((3 * r + 3) & ~3) - 3 * r for r in fc.SHARPEN_RADII} == {0, 1, 2, 3}


def test_the_taps_of_every_radius():
    """sharpen_cases.taps_of at a sigma whose radius is R, for every R: R + 1 taps that add up to 32768, none of them 0 up to R = 12 at least;
    and the hand-made set that does not fall with the distance."""
    for R in fc.SHARPEN_RADII:
        taps = fc.radius_taps(R)
        assert len(taps) == R + 1 and taps[0] + 2 * sum(taps[1:]) == sc.ONE and taps[1] > 0 and all(0 <= t < 65536 for t in taps)
    t = fc.ODD_TAPS
    assert t[0] + 2 * sum(t[1:]) == sc.ONE and t[1] < t[2] > t[3] and len(set(t)) == 4


# -- enlarge's full LDS row ------------------------------------------------------------------------------
def test_enlarge_fills_its_lds_row_and_its_staged_rectangle():
    """A tile of 64 targets at a ratio just above 1 that no position skips lies at 64 positions in a row: taps over 67 patch pixels, and with
    a half-pixel start 68 raw pixels, 204 bytes, which 3 bytes of shift make the 52 dwords of an LDS row; likewise 16 + 3 + 1 = 20 rows.
    The first call reaches both at every src_shift, in its middle tile; the second, on whole pixels, 67 pixels and 19 rows.  In both the
    first tile's span is cut by the clamp at the patch's first pixel and the last one's by the clamp at its last, on both axes."""
    assert (fc.RAW_PX, fc.RAW_ROWS) == (68, 20) and (3 + 3 * fc.RAW_PX + 3) // 4 == 52
    for i, ((W, H), crop, size) in enumerate(fc.FULL_ROWS):
        half = (cc.start(W, crop[0])[1], cc.start(H, crop[1])[1])
        assert half == ((True, True), (False, False))[i] and size[0] <= 3 * 64 and size[1] <= 48
        stride = 3 * W + fc.full_row_case(i)[1]['pad']
        assert stride % 2 == 1
        for src_shift in fc.SRC_SHIFTS:
            _, longest, most = fc.enlarge_fetch_classes(W, H, crop, size, stride, src_shift)
            assert (longest, most) == (((68, 3), 20), ((67, 3), 19))[i], (i, src_shift)
        for n_in, n_out, tile in ((crop[0], size[0], 64), (crop[1], size[1], 16)):
            cuts, spans = fc.enlarge_cuts(n_in, n_out, tile), fc._enlarge_spans(n_in, n_out, tile)
            assert len(cuts) == 3 and cuts == [(True, False), (False, False), (False, True)]
            assert spans[1][1] - spans[1][0] == tile + 3 and all(b - a < tile + 3 for a, b in (spans[0], spans[2]))


# -- the twins at the sweeps' shapes -------------------------------------------------------------------------
def test_the_sharpen_twin_is_the_header_at_every_radius():
    """Every frame of every radius, the hand-made taps, and widths of the store sweep at both of its radii."""
    for R in fc.SHARPEN_RADII:
        for frame in fc.sharpen_radius_frames(R):
            (frames, taps, amount), _, want = fc.sharpen_radius_case(R, frame)
            assert np.array_equal(sc.header_sharpen(frames, taps, amount, pad=1), want), (R, frame)
    R = len(fc.ODD_TAPS) - 1
    for frame in fc.sharpen_radius_frames(R):
        (frames, taps, amount), _, want = fc.sharpen_radius_case(R, frame, fc.ODD_TAPS)
        assert taps == fc.ODD_TAPS and not np.array_equal(want, fc.sharpen_radius_case(R, frame)[2])
        assert np.array_equal(sc.header_sharpen(frames, taps, amount, pad=1), want), frame
        swapped = (taps[0], taps[2], taps[1], taps[3])
        assert not np.array_equal(sc.twin_sharpen(frames, swapped, amount), want)                       # (a tap taken at another distance shows)
    for entry, R in fc.STORE_SWEEPS:
        if entry == 'sharpen':
            for w in (1, 21, 64, 130):
                (frames, taps, amount), _, want = fc.store_case(entry, R, w)
                assert np.array_equal(sc.header_sharpen(frames, taps, amount), want), (R, w)
    for W in fc.FETCH_WIDTHS['sharpen'][:2]:
        (frames, taps, amount), _, want = fc.fetch_case('sharpen', 7, W)
        assert np.array_equal(sc.header_sharpen(frames, taps, amount), want), W


def test_the_enlarge_twin_is_the_header_at_the_sweeps_shapes():
    """The calls that fill the LDS row, and widths of the store and the fetch sweep on both routes."""
    for i in range(len(fc.FULL_ROWS)):
        (frames, crop, size), _, want = fc.full_row_case(i)
        assert np.array_equal(ec.header_enlarge(frames, crop, size, pad=1), want), i
    for variant in ('oo', 'ee'):
        for w in (1, 2, 43, 64, 130):
            (frames, crop, size), _, want = fc.store_case('enlarge', variant, w)
            assert np.array_equal(ec.header_enlarge(frames, crop, size), want), (variant, w)
        (frames, crop, size), _, want = fc.fetch_case('enlarge', variant, fc.FETCH_WIDTHS['enlarge'][0])
        assert np.array_equal(ec.header_enlarge(frames, crop, size), want), variant


# -- the exact reduction by prefix sums ------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ac.TARGETS))
def test_the_prefix_sums_are_the_twin(name):
    assert np.array_equal(fc.exact_reduce(ac.photo(3), *ac.TARGETS[name]), ac.twin_of(name, 3))


def test_the_prefix_sums_are_the_crop_twin():
    W, H = cc.FRAMES[2]
    for name in sorted(cc.OFF):
        crop = cc.crop_of((W, H), name)
        for size in cc.targets(crop).values():
            assert np.array_equal(fc.exact_crop_reduce(cc.frames(W, H), crop, size), cc.twin_of(W, H, crop, size)), (name, size)


@pytest.mark.parametrize('name', fc.LIMITS)
def test_the_prefix_sums_are_the_header_at_the_sides_limit(name):
    """65535 x 2 and 2 x 65535, where span_end works within 0.002 % of 2^32 and the twin's weight matrix cannot be built."""
    frame = fc.limit_frame(name)
    assert frame.shape[1:] == {'widest': (2, 65535, 3), 'tallest': (65535, 2, 3)}[name]
    for w, h in fc.area_limit_targets(name):
        assert np.array_equal(fc.exact_reduce(frame, w, h), ac.header_reduce(frame, w, h)), (w, h)


@pytest.mark.parametrize('name', fc.LIMITS)
def test_the_prefix_sums_are_the_crop_header_at_the_sides_limit(name):
    frame = fc.limit_frame(name)
    cases = fc.crop_limit_cases(name)
    assert len(cases) == 9 and {(cc.start(frame.shape[2], cw)[1], cc.start(frame.shape[1], ch)[1]) for (cw, ch), _ in cases} == {(False, False), (True, True), (name == 'widest', name == 'tallest')}
    for crop, size in cases:
        assert np.array_equal(fc.exact_crop_reduce(frame, crop, size), cc.header_reduce(frame, crop, size)), (crop, size)


@pytest.mark.parametrize('axis', ['x', 'y'])
def test_the_header_is_the_prefix_sums_at_random_ratios(axis):
    """150 seeded (N, n) pairs up to 65535 along one axis, the other 2 -> 1 or 2 -> 2: the pairs at the limit and next to it among them."""
    rng = np.random.default_rng(11 if axis == 'x' else 12)
    pairs = [(65535, 65535), (65535, 65534), (65535, 1), (65534, 65533), (65535, 32768), (65535, 32767)]
    while len(pairs) < 150:
        N = int(rng.integers(1, 65536)) if len(pairs) % 3 else int(rng.integers(1, 300))
        pairs.append((N, int(rng.integers(1, N + 1))))
    for i, (N, n) in enumerate(pairs):
        line = rng.integers(0, 256, (1, 2, N, 3), dtype=np.uint8)
        if i % 4 == 0:
            line[:] = 255                                                 # (the largest sums)
        frame, size = (line, (n, 1 + i % 2)) if axis == 'x' else (np.ascontiguousarray(line.transpose(0, 2, 1, 3)), (1 + i % 2, n))
        assert np.array_equal(ac.header_reduce(frame, *size), fc.exact_reduce(frame, *size)), (N, n)


# -- the blur at the sides' limit ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', fc.LIMITS)
def test_the_blur_header_is_the_twin_at_the_ends_of_the_sides_limit(name):
    """The GPU test holds the device to the header's bytes there (the twin takes 5 to 15 s on such a frame).  Here the twin blurs the first and
    the last 1500 pixels of the long side as frames of their own: away from the cut, beyond the reach of R = 16, its bytes are the header's."""
    frame, depth, want = fc.limit_frame(name), fc.limit_depth(name), fc.limit_blur(name)
    assert (want != frame).mean() > 0.3
    axis = 2 if name == 'widest' else 1
    for end, kept in ((slice(0, 1500), slice(0, 1500 - 16)), (slice(65535 - 1500, 65535), slice(16, 1500))):
        cut = [slice(None)] * 3
        cut[axis] = end
        twin = dc.twin_blur(frame[tuple(cut)], depth[tuple(cut)], dc.focus_of(1), dc.APERTURE, 16)
        keep = [slice(None)] * 3
        keep[axis] = kept
        assert np.array_equal(twin[tuple(keep)], want[tuple(cut)][tuple(keep)]), end


# -- the radius --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', fc.RADIUS_ORDER)
def test_a_marked_frame_shows_its_radii(name):
    """The twin and the header agree on the marks' radii and those are the stated ones; the twin's bytes are the closed form's and would be
    others at a radius one off (filter_sweep_cases.radius_case); and the header's blur is the twin's."""
    frame, depth, want = fc.radius_case(name)
    zf, A = fc.RADIUS_CASES[name][:2]
    assert np.array_equal(dc.header_blur(frame, depth, [zf], A, 16), want)


def test_the_marks_lie_on_both_sides_of_the_tiles_borders():
    assert (fc.MARK_W, fc.MARK_H) == (128, 32)
    for layout in fc.LAYOUTS:
        xs = sorted(x for x, _ in layout)
        assert all(b - a >= 33 + 2 for a, b in zip(xs, xs[1:])) and all(17 <= x <= fc.MARK_W - 18 for x in xs)          # 3 x 3 blocks, 33 and more apart, their discs inside the frame
    assert {x for layout in fc.LAYOUTS for x, _ in layout} >= {63, 64} and {y for layout in fc.LAYOUTS for _, y in layout} == {15, 16}
    # every mark of the ties comes to lie on a border column in some case
    for k in range(3):
        assert {fc.mark_places(name)[k][0] for name in fc.RADIUS_ORDER if name.startswith('tie')} >= {63, 64}
