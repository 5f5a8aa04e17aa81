"""CPU checks behind the table-driven hole fill (k_hole_dist, k_fill_tables of ken-burns-effect_amd/csrc/kbe_holes.hip): its exact
arithmetic and launch_fill's decisions live in csrc/kbe_fill_walk.h, which hipcc compiles into the kernels and g++ compiles into
tests/fill_walk_check.cpp -- the functions checked here against brute force are the ones the kernels run (no GPU, no oracle):
  * m fp32 additions of a fill direction taken on the integer mantissa (axis_jump, axis_catch_up, advance_exact) against the
    additions one at a time (common.py:876-889): bits and pixels identical;
  * the strip test (strip_bounds, strip_skip) against brute-force walks on a mask: no direction that completes (both ends reach a
    valid pixel before leaving the image, common.py:880-896) is ever skipped; k_dead and the jump lengths on the same walks;
  * the contest key and fill_plan against the written rule."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_LANE, PER_HALFWAVE, BY_COUNT, DIST = 8, 16, 32, 512     # include/kbe.h: KBE_STAGE_FILL_*
SERIAL_MIN = 49152                                          # kbe_fill_walk.h: KBE_FILL_SERIAL_MIN


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('fill_walk') / 'fill_walk_check')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc'),
                           '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'fill_walk_check.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def strip_report(checker, tmp_path_factory):
    """A zoomed-out frame in miniature: a trapezoid with a ragged, speckled rim and a tower beside it."""
    rng = np.random.default_rng(5)
    H = W = 1024
    yy, xx = np.mgrid[0:H, 0:W]
    half = 120 + (yy - 300) * 0.45
    mask = (yy >= 300) & (yy < 880) & (np.abs(xx - 500) < half)
    mask |= (xx >= 720) & (xx < 880) & (yy < 270)
    rim = (yy >= 290) & (yy < 900) & (np.abs(np.abs(xx - 500) - half) < 25)
    mask = np.where(rim, rng.random((H, W)) < 0.3, mask)
    mask[400:420, 380:520] = False                                   # a hole inside: directions complete here
    path = str(tmp_path_factory.mktemp('fill_mask') / 'mask.u8')
    mask.astype(np.uint8).tofile(path)
    out = subprocess.run([checker, 'strips', path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    return out.stdout


def test_many_fp32_additions_at_once_equal_the_additions_one_at_a_time(checker):
    out = subprocess.run([checker, 'advance'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    m = re.search(r'walks (\d+), advances (\d+) \(catch-ups (\d+)\), mismatches (\d+)', out.stdout)
    assert m and int(m.group(4)) == 0 and int(m.group(2)) > 1000000 and int(m.group(3)) > 100000, out.stdout[-500:]
    # the walks start at 0 .. 11000, the longest side the tables take: every pixel up to 1100, around 8192 -- where a binade begins -- and
    # of the last dozen, every seventh between; 32 steps in either sense (with starts up to 9000 only they were 142 656 walks)
    assert int(m.group(1)) == 32 * 2 * (1100 + 1011 + 31 + 397 + 14)
    t = re.search(r'ties: walks (\d+), advances (\d+) \(catch-ups (\d+)\), mismatches (\d+)', out.stdout)       # steps that round to even
    assert t and int(t.group(4)) == 0 and int(t.group(2)) > 1000000, out.stdout[-500:]


def test_strip_test_never_skips_a_direction_that_completes(strip_report):
    m = re.search(r'complete (\d+) .*survive strip test (\d+) .*false kills (\d+)', strip_report)
    assert m, strip_report[-500:]
    complete, survive, false_kills = (int(g) for g in m.groups())
    assert false_kills == 0 and complete > 100000 and survive >= complete
    pairs = int(re.search(r'pairs (\d+)', strip_report).group(1))
    assert survive < 0.6 * pairs, 'the test skips a good share of the directions at once'
    assert int(re.search(r'bins out of range (\d+)', strip_report).group(1)) == 0


def test_an_end_past_k_dead_never_meets_a_valid_pixel(strip_report):
    m = re.search(r'dead ends (\d+), steps walked beyond (\d+), valid pixels met (\d+)', strip_report)
    assert m, strip_report[-500:]
    ends, steps, met = (int(g) for g in m.groups())
    assert met == 0 and ends > 100000 and steps > 10 * ends, strip_report[-1000:]


def test_no_position_skipped_by_a_jump_is_valid(strip_report):
    m = re.search(r'jump walks (\d+), positions skipped (\d+), valid pixels skipped (\d+), jumps of no step (\d+)', strip_report)
    assert m, strip_report[-500:]
    walks, skipped, bad, stuck = (int(g) for g in m.groups())
    assert bad == 0 and stuck == 0 and walks > 100000 and skipped > 10 * walks, strip_report[-1000:]


def test_strip_bounds_of_a_lone_tile_are_those_of_its_valid_pixels(checker):
    """The tile whose box reaches farthest is looked at pixel by pixel: with one tile the bounds are exact, whatever its box."""
    out = subprocess.run([checker, 'tile'], capture_output=True, text=True, timeout=60)
    m = re.search(r'one tile: empty strips (\d+) \(bounded all the same (\d+)\), strips with a pixel (\d+) \(not bounded by it (\d+)\)', out.stdout)
    assert out.returncode == 0 and m, out.stdout[-1000:]
    empty, empty_bounded, holding, holding_wrong = (int(g) for g in m.groups())
    assert empty_bounded == 0 and holding_wrong == 0 and empty > 10000 and holding >= 16 * 2 * 2


def test_contest_key_round_trips_and_orders_by_length_then_direction(checker):
    out = subprocess.run([checker, 'key'], capture_output=True, text=True, timeout=60)
    m = re.search(r'key: entries (\d+), round trips bad (\d+), pairs compared (\d+), order bad (\d+)', out.stdout)
    assert out.returncode == 0 and m, out.stdout[-500:]
    entries, bad_trips, compared, bad_order = (int(g) for g in m.groups())
    assert bad_trips == 0 and bad_order == 0 and entries >= 10000 and compared > 100000


def ceil_div(a, b):
    return -(-a // b)


def test_fill_plan_follows_the_stage_bits_and_the_frame_size(checker):
    """launch_fill's decisions by the written rule (include/kbe.h: KBE_STAGE_FILL_*)."""
    sizes = [(512, 512), (1024, 1024), (2048, 2048), (1000, 562), (12000, 512), (40, 30),
             (40, 8192), (40, 8208), (33, 11000), (33, 11001), (16416, 48)]           # (tests/elongated_cases.py: either side of 512 tile rows and of 11 000 pixels)
    cases = []
    for (W, H), bits in itertools.product(sizes, itertools.product((0, 1), repeat=4)):
        stages = sum(b * f for b, f in zip(bits, (PER_LANE, PER_HALFWAVE, BY_COUNT, DIST))) | 1 | 64       # other stage bits do not matter
        cases.append((W, H, stages, ceil_div(W, 32), ceil_div(H, 16)))
    cases.append((1024, 1024, PER_LANE | DIST, 513, 64))            # more tile columns than the strip tables take
    text = ''.join('%d %d %d %d %d\n' % c for c in cases)
    out = subprocess.run([checker, 'plan'], input=text, capture_output=True, text=True, check=True)
    rows = [line.split() for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    seen_tables = 0
    for (W, H, stages, tx, ty), row in zip(cases, rows):
        mode, tables, min_holes, use_strips, gx, gy, image_rows, tables_blocks, fill_blocks, arg = (int(v) for v in row[:10])
        left = row[10]
        lane, half, count, dist = (bool(stages & f) for f in (PER_LANE, PER_HALFWAVE, BY_COUNT, DIST))
        assert mode == (1 if lane else 2 if half or not count else 0), (W, H, stages)
        assert fill_blocks == min(max(W * H // 64, 1), 2048)
        want_tables = dist and (lane or count) and W <= 11000 and H <= 11000
        assert bool(tables) == want_tables, (W, H, stages)
        if not want_tables:
            assert arg == 0 and left == '111'                       # k_fill_holes fills every frame
            continue
        seen_tables += 1
        assert min_holes == (0 if lane else SERIAL_MIN)
        assert use_strips == (1 if tx <= 512 and ty <= 512 else 0)
        assert arg == 1 + min_holes and left == '100'               # ... the frames with fewer than min_holes holes
        assert (gx, image_rows) == (ceil_div(W, 64), ceil_div(H, 32))
        extra = 16 * ceil_div(W + H + 8, 256) + ceil_div(tx * 4, 64) * ceil_div(ty * 2, 32)     # strip tables, then the block table
        assert gy == image_rows + ceil_div(extra, gx)
        assert tables_blocks == min(ceil_div(W * H, 256), 768)
    assert seen_tables >= 20
