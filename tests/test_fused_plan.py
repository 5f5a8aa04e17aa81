"""What the fused scatter's launch decides on the host (ken-burns-effect_amd/csrc/kbe_fused_plan.h: plain C++ on plain values): which
consecutive frames share candidate lists, whether a tile launch carries the next one's placements, and which kernel it is.  The C++
checker next to this file prints single decisions and sweeps the plan's structure; the expected values here come from the written rule
 and from arithmetic done in this file."""
import math
import os
import subprocess

import numpy as np
import pytest

from ken_burns_effect_amd import common

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, os.pardir, 'ken-burns-effect_amd', 'csrc')
SHARE_MAX_PX = 13.0                 # kbe_fused_plan.h: KBE_SHARE_MAX_PX
SIZES = (12, 8, 6, 4)
BENCH_N, BENCH_W = 1137109, 1024    # the bench cloud
SINGLE, SINGLE_AHEAD, GROUP, GROUP_AHEAD = range(4)
LEAN, ROOMY, DENSE = range(3)


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('fused_plan') / 'fused_plan_check')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-I', CSRC, os.path.join(HERE, 'fused_plan_check.cpp'), '-o', exe])
    return exe


def f32(v):
    return float(np.float32(v))


def share(checker, cams, near_depth, m=None, N=BENCH_N, W=BENCH_W, H=BENCH_W):
    """cams: [(focal, (sx, sy, sz))] or [(focal, shift3, has_shift)] -> (any, dev[3], sub-group sizes in order, raw rows)"""
    m = len(cams) if m is None else m
    text = ''.join('%r %r %r %r %d\n' % (c[0], f32(c[1][0]), f32(c[1][1]), f32(c[1][2]), c[2] if len(c) > 2 else 1) for c in cams)
    out = subprocess.run([checker, 'share', str(N), str(W), str(H), repr(float(near_depth)), str(m)], input=text, capture_output=True, text=True, check=True)
    lines = out.stdout.splitlines()
    head = lines[0].split()
    rows = [tuple(int(v) for v in line.split()) for line in lines[1:]]
    assert len(rows) == 12
    sizes, k = [], 0
    while k < m:
        lead, last, size = rows[k]
        assert lead == k and size == last - lead + 1 and all(rows[j] == rows[k] for j in range(k, last + 1))
        sizes.append(size)
        k = last + 1
    assert all(rows[k] == (k, k, 1) for k in range(m, 12))
    return bool(int(head[0])), [float(v) for v in head[1:]], sizes, rows


def identity(result, m):
    any_, dev, sizes, _ = result
    return not any_ and dev == [0.0, 0.0, 0.0] and sizes == [1] * m


def straight(p, F=512.0, zn=100.0, n=12):
    """n cameras of focal F on a straight line in x, equal steps, under which a point at depth zn moves p pixels per step"""
    dx = p * zn / F
    return [(F, (f32(dx * k), 0.0, 0.0)) for k in range(n)]


def pick(checker, N, W, H, n, n_next, forced=0):
    out = subprocess.run([checker, 'pick'] + [str(v) for v in (N, W, H, n, n_next, forced)], capture_output=True, text=True, check=True)
    units, can, shape, build = (int(v) for v in out.stdout.split())
    return units, bool(can), shape, build


@pytest.mark.parametrize('p, sizes', [(1.0, [12]), (1.5, [8, 4]), (2.0, [6, 6]), (3.0, [4, 4, 4]), (5.0, [])])
def test_share_rule_on_straight_equal_step_paths(checker, p, sizes):
    """The largest sub-group size s of 12, 8, 6, 4 whose first and last camera move the nearest point by (s - 1) p <= 13 pixels; each p
    leaves at least a pixel to 13 on both sides: 11 | 16.5, 10.5 | 14, 10 | 15, 9 | 15."""
    s = next((s for s in SIZES if (s - 1) * p <= SHARE_MAX_PX), None)
    assert s is None or ((s - 1) * p <= SHARE_MAX_PX - 1.0 and all((t - 1) * p >= SHARE_MAX_PX + 1.0 for t in SIZES if t > s))
    assert s is not None or 3 * p >= SHARE_MAX_PX + 1.0
    assert sizes == ([] if s is None else [s] * (12 // s) + ([12 % s] if 12 % s else []))
    cams = straight(p)
    any_, dev, got, _ = share(checker, cams, 100.0)
    if not sizes:
        assert identity((any_, dev, got, None), 12)
        return
    assert any_ and got == sizes
    # a straight path stays on its chords: dev is the rounding floor, 2e-6 of the largest shift and the fp32 rounding of the shifts
    big = max(abs(c[1][0]) for c in cams)
    assert big > 1.0 and all(2.0e-6 * big <= d <= 3.0e-6 * big for d in dev), dev


def kb_scene(dolly=False):
    """A zoom to three quarters of the image with a sideways move, 1024^2, focal 1024, the closest point at depth 200."""
    oc = {'intWidth': 1024, 'intHeight': 1024, 'dblFocal': 1024.0, 'dblBaseline': 40.0, 'objectDepthrange': [200.0, 3000.0, (400.0, 600.0)]}
    settings = {'objectFrom': {'dblCenterU': 512.0, 'dblCenterV': 512.0, 'intCropWidth': 1024, 'intCropHeight': 1024},
                'objectTo': {'dblCenterU': 560.0, 'dblCenterV': 500.0, 'intCropWidth': 768, 'intCropHeight': 768}, 'dolly': dolly}
    return settings, oc


def spread_px(a, b, near_depth, F, half):
    """how far the nearest point moves between two cameras (shifts a, b), in pixels -- sideways by the shift's
    motion x F, in depth by at most half the image x the change of sz, both over the depth it is left at"""
    zn = near_depth + min(a[2], b[2])
    assert zn > 0.01 * F
    return (math.hypot(b[0] - a[0], b[1] - a[1]) * F + half * abs(b[2] - a[2])) / zn


@pytest.mark.parametrize('steps, sizes', [(400, [12]), (85, [6, 6]), (20, [])])
def test_share_plan_fires_on_a_ken_burns_path(checker, steps, sizes):
    """The first twelve cameras of the product's own path -- a parabola in shift space, common.py:88-100 -- at three step counts:
    whole launches share, sub-groups share, lists per frame.  (Round 4's rule asked for a straight line and never fired on such a path;
    the GPU tests compare frames with sharing on and off, which holds as well when nothing is shared: DESIGN.md section 4.4.)"""
    settings, oc = kb_scene()
    cams = common.frame_cameras(dict(settings, dblSteps=[i / (steps - 1.0) for i in range(12)]), oc)
    near, F, half = oc['objectDepthrange'][0], oc['dblFocal'], 512.0
    assert all(c[0] == F for c in cams)
    sh = [c[1] for c in cams]
    # the rule, restated: the largest size whose every sub-group fits; no comparison that decides is closer than half a pixel
    want = None
    for s in SIZES:
        spreads = [spread_px(sh[a0], sh[min(a0 + s, 12) - 1], near, F, half) for a0 in range(0, 12, s)]
        assert all(abs(v - SHARE_MAX_PX) > 0.5 for v in spreads), spreads
        if want is None and max(spreads) <= SHARE_MAX_PX:
            want = [min(a0 + s, 12) - a0 for a0 in range(0, 12, s)]
    assert (want or []) == sizes
    any_, dev, got, rows = share(checker, cams, near)
    if not sizes:
        assert identity((any_, dev, got, None), 12)
        return
    assert any_ and got == sizes
    # a parabola strays from its chords: every component above the rounding floor, every camera within dev of its sub-group's chord
    # (the point of the chord nearest to it), and by less than the 2 pixels beyond which the plan declines
    big = max(1.0, max(abs(v) for s in sh for v in s))
    assert all(d > 10 * 2.0e-6 * big for d in dev), dev
    for k, (lead, last, _) in enumerate(rows):
        d = [sh[last][q] - sh[lead][q] for q in range(3)]
        e = [sh[k][q] - sh[lead][q] for q in range(3)]
        lam = min(max(sum(e[q] * d[q] for q in range(3)) / sum(v * v for v in d), 0.0), 1.0)
        assert all(abs(e[q] - lam * d[q]) <= dev[q] for q in range(3)), (k, dev)
    assert (math.hypot(dev[0], dev[1]) * F + half * dev[2]) / (near + min(sh[0][2], sh[11][2])) < 2.0


def test_share_plan_declines_what_it_must(checker):
    base = straight(1.0)
    assert share(checker, base, 100.0)[2] == [12]
    assert identity(share(checker, base, 0.0), 12)                      # no near depth: the run-time off switch (KBE_SHARE_LISTS=0)
    back = [(c[0], (c[1][0], 0.0, 100.0)) for c in base]               # (... whatever the cameras' own sz leaves in front of them)
    assert share(checker, back, 100.0)[2] == [12] and identity(share(checker, back, 0.0), 12)
    for m in (0, 1, 2, 3):
        assert identity(share(checker, base, 100.0, m=m), m)            # fewer than four frames: lists of their own
    assert share(checker, base, 100.0, m=4)[2] == [4]
    for k in (0, 5, 11):
        assert identity(share(checker, [c + (0,) if i == k else c for i, c in enumerate(base)], 100.0), 12)     # a camera without shift
        assert identity(share(checker, [(c[0] + 1.0, c[1]) if i == k else c for i, c in enumerate(base)], 100.0), 12)   # another focal length
    # shifts above 100 (fp32 leaves too little of them): the same path 99 and 100.5 to the side
    assert share(checker, [(c[0], (c[1][0], 99.0, 0.0)) for c in base], 100.0)[2] == [12]
    assert identity(share(checker, [(c[0], (c[1][0], 100.5, 0.0)) for c in base], 100.0), 12)
    # a path that strays from its chord by more than 2 pixels at the nearest depth (the cameras between the first and the last a step
    # aside: 1 px shares, 3 px does not), though its first and last camera are 11 px apart as before
    aside = lambda px: [(c[0], (c[1][0], f32(px * 100.0 / 512.0) if 0 < i < 11 else 0.0, 0.0)) for i, c in enumerate(base)]
    assert share(checker, aside(1.0), 100.0)[2] == [12]
    assert identity(share(checker, aside(3.0), 100.0), 12)
    # a dolly zoom changes the focal length from frame to frame (common.py:185-188)
    settings, oc = kb_scene(dolly=True)
    cams = common.frame_cameras(dict(settings, dblSteps=[i / 399.0 for i in range(12)]), oc)
    assert len(set(c[0] for c in cams)) == 12
    assert identity(share(checker, cams, oc['objectDepthrange'][0]), 12)
    settings, oc = kb_scene()
    assert share(checker, common.frame_cameras(dict(settings, dblSteps=[i / 399.0 for i in range(12)]), oc), oc['objectDepthrange'][0])[2] == [12]
    # a cloud whose average list (1.55 candidates per point of a tile's share, in sub-blocks of 16) exceeds a quarter of the 2048 a
    # list holds: 16.8 M points on 2048^2 (64 x 128 tiles) 198 <= 512 shares, four times the points do not
    assert 1.55 * 16777216 / 16 / 8192 < 512 < 1.55 * 4 * 16777216 / 16 / 8192
    assert share(checker, base, 100.0, N=16777216, W=2048, H=2048)[2] == [12]
    assert identity(share(checker, base, 100.0, N=4 * 16777216, W=2048, H=2048), 12)


def test_share_plan_structure(checker):
    """Random straight, curved and noisy paths of every scale, some with a camera that rules sharing out, m = 0..12: sub-groups are
    consecutive and tile [0, m), lead <= k <= last, size matches, slots >= m are their own, and the launch that places a group and the
    launch that renders it -- the same cameras inside different records -- get the same plan."""
    out = subprocess.run([checker], capture_output=True, text=True)
    plans, failures, sharing = (int(v) for v in out.stdout.split())
    assert out.returncode == 0 and failures == 0 and plans >= 50_000 and sharing >= plans // 10 and plans - sharing >= plans // 10, out.stderr


def test_kernel_pick(checker):
    """From the documents' own figures (kbe_fused.hip)."""
    # the bench cloud, twelve frames that place twelve: 17 768 units of 64 points over 2048 tiles x 4 waves = 2.17, rounded up
    assert math.ceil(math.ceil(BENCH_N / 64) * 12 / (2048 * 4 * 12)) == 3
    assert pick(checker, BENCH_N, 1024, 1024, 12, 12) == (3, True, GROUP_AHEAD, LEAN)
    assert pick(checker, BENCH_N, 1024, 1024, 12, 12, forced=2) == (3, True, GROUP_AHEAD, ROOMY)
    assert pick(checker, BENCH_N, 1024, 1024, 12, 0)[2:] == (GROUP, LEAN)
    assert pick(checker, BENCH_N, 1024, 1024, 12, 0, forced=2)[2:] == (GROUP, ROOMY)
    # lean up to 1.125 points per pixel
    assert pick(checker, 1179648, 1024, 1024, 12, 12)[3] == LEAN and pick(checker, 1179648 + 1, 1024, 1024, 12, 12)[3] == ROOMY
    assert pick(checker, 1179648 + 1, 1024, 1024, 12, 12, forced=1)[3] == LEAN
    # 16.8 M points on 2048^2, three frames that place three: 8 units per wave, the dense launch -- which has one build
    assert 16777216 // 64 * 3 // (8192 * 4 * 3) == 8
    for forced in (0, 1, 2):
        assert pick(checker, 16777216, 2048, 2048, 3, 3, forced) == (8, True, GROUP_AHEAD, DENSE)
    # dense from five units per wave on (KBE_AHEAD_UNITS + 1 = 4 are the group launch's): 4 and 4 + one block of 64 points more
    assert pick(checker, 4 * 8192 * 64, 1024, 1024, 12, 12) == (4, True, GROUP_AHEAD, ROOMY)
    assert pick(checker, 4 * 8192 * 64 + 1, 1024, 1024, 12, 12) == (5, True, GROUP_AHEAD, DENSE)
    # one frame that places at most one: the FrameJob1 kernels; one that places several is a group launch
    assert pick(checker, BENCH_N, 1024, 1024, 1, 0)[2:] == (SINGLE, LEAN)
    assert pick(checker, BENCH_N, 1024, 1024, 1, 1)[2:] == (SINGLE_AHEAD, LEAN)
    assert pick(checker, BENCH_N, 1024, 1024, 1, 0, forced=2)[2:] == (SINGLE, ROOMY)
    assert pick(checker, BENCH_N, 1024, 1024, 1, 2)[2] == GROUP_AHEAD
    # placements ahead up to nine units per wave: 9 x 8192 x 64 points on 1024^2, and one block more
    assert pick(checker, 9 * 8192 * 64, 1024, 1024, 12, 12)[:2] == (9, True)
    assert pick(checker, 9 * 8192 * 64 + 1, 1024, 1024, 12, 12)[:2] == (10, False)
    assert pick(checker, BENCH_N, 1024, 1024, 1, 12)[:2] == (math.ceil(17768 * 12 / 8192), False)       # 27 units
    assert not pick(checker, BENCH_N, 1024, 1024, 12, 0)[1] and not pick(checker, BENCH_N, 1024, 1024, 0, 12)[1]
