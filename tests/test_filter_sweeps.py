"""What tests/test_filter_sweeps_gpu.py rests on, without a GPU (tests/filter_sweep_cases.py): the sweeps' parameters reach every alignment class
of the tile store and row fetch that the kernels share (csrc/kbe_rows.h), by the launch arithmetic alone; that header itself, executed
serially (tests/rows_check.cpp); the exact area reduction by prefix sums equals the headers and the twins wherever both exist, the sides'
limit among them; and every frame that makes a radius visible is sensitive to it."""
import re
import subprocess

import numpy as np
import pytest

import area_cases as ac
import crop_area_cases as cc
import dof_cases as dc
import filter_sweep_cases as fc
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
    the widths; area's sweep at ratio 1 takes at least eight widths, each at every lead."""
    found = fc.store_sweep_classes(entry, variant)
    widths = fc.store_widths(entry, variant)
    if (entry, variant) == ('area', 'copy'):
        assert len(widths) >= 8 and found == {(lead, min(w - ox0, 64)) for w in widths for ox0 in range(0, w, 64) for lead in range(16)}
    else:
        assert set(range(1, 65)) <= set(widths) and {65, 127, 128, 129} <= set(widths)
        assert found == fc.EVERY_STORE_CLASS and len(found) == 1024
    assert all(fc.store_stride(w) % 2 == 1 and fc.store_stride(w) > 3 * w for w in widths)           # odd, and with padding that must stay unwritten


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
