"""What tests/test_hip_elongated.py runs on: rasters far from square, each chosen for the code path that ONE of its sides selects
(include/kbe.h promises sides up to 2^23 for the frame loop, 65535 for the encoders, any W, H > 0 for the glue kernels), the
scenes on them, and the hole-fill plan each of them takes (csrc/kbe_fill_walk.h: fill_plan, through tests/fill_walk_check.cpp).
Plain values and a scene builder: nothing here needs a GPU."""
import collections
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOCAL, BASELINE = 512.0, 120
TILE_W, TILE_H = 32, 16                                     # csrc/kbe_tiles.h: KBE_TILE_W, KBE_TILE_H
STRIP_TILES = 512                                           # csrc/kbe_fill_walk.h: the strip tables take up to this many tile rows / columns
TABLES_MAX_SIDE = 11000                                     # csrc/kbe_fill_walk.h: fill_tables_fit
MORTON_CLAMP_W = 65504                                      # csrc/kbe_cloud.hip: the Morton cell of kbe_cloud_pack clamps at 8190 (8 x 8190 - 16 pixels)
DEVICE_BUDGET = 1 << 30                                     # no test allocates more device memory than this
PER_LANE, PER_HALFWAVE, BY_COUNT, DIST = 8, 16, 32, 512     # include/kbe.h: KBE_STAGE_FILL_*

# a frame of the frame loop: the raster, the scene (synthetic.make_rgbd's kind and seed), the camera's shift3, and what it is there for
FrameCase = collections.namedtuple('FrameCase', 'name H W kind seed shift3 why')
FRAME_CASES = [
    FrameCase('48x16416', 48, 16416, 'smooth', 3, (6.0, -3.0, -40.0), '513 tile columns'),
    FrameCase('8208x40', 8208, 40, 'smooth', 3, (3.0, -6.0, 30.0), '513 tile rows, a partial tile column, rows that are all holes'),
    FrameCase('8208x40_noise', 8208, 40, 'noise', 3, (3.0, -6.0, 30.0), 'the same raster, white-noise depth'),
    # (no camera here shifts in y by a row or more: a row of holes makes the ORACLE's fill walk the long side once per hole)
    FrameCase('5x70016_in', 5, 70016, 'smooth', 3, (6.0, 0.4, 25.0), 'one partial tile row; W beyond the Morton clamp; columns that are all holes'),
    FrameCase('5x70016_out', 5, 70016, 'smooth', 3, (6.0, 0.4, -25.0), 'the same raster, the camera moving back'),
    FrameCase('11000x33', 11000, 33, 'smooth', 3, (2.0, -3.0, -40.0), 'the last size the fill tables take'),
    FrameCase('11001x33', 11001, 33, 'smooth', 3, (2.0, -3.0, 30.0), 'the first size they refuse'),
    FrameCase('8192x40', 8192, 40, 'smooth', 3, (3.0, -6.0, 30.0), '512 tile rows: the last size with strip tables'),
]
FRAME = {c.name: c for c in FRAME_CASES}
ORACLE_CASES = [c.name for c in FRAME_CASES if c.name != '8192x40']       # section A of the suite; 8192x40 is the fill's (the other side of 8208)

# the fill schedules on the same un-filled frame: case -> (tables, use_strips) of PER_LANE | DIST as fill_plan decides it (None: no tables, no plan)
FILL_CASES = {'8208x40': (1, 0),         # tables without their strips: more than STRIP_TILES tile rows
              '8192x40': (1, 1),         # ... and with them, one tile row fewer
              '11000x33': (1, 0),        # the last size with tables (688 tile rows: no strips either)
              '11001x33': (0, None),     # H > 11 000: the flag is ignored
              '48x16416': (0, None)}     # W > 11 000: the flag is ignored
FILL_MODES = (0, PER_LANE, PER_HALFWAVE, PER_LANE | DIST)   # default, one lane per hole, one half-wave per hole, one lane per hole with the tables (min_holes = 0)
GROUP_CASES = ['48x16416', '8208x40']
CROPS = {'48x16416': (14774, 43), '8208x40': (36, 7387)}    # (crop_w, crop_h): nine tenths of either side

DEGRID_SERIAL_SHAPES = [(1500, 24), (2100, 3)]              # (H, W): more rows than the 1024 threads of k_degrid_serial's workgroup
FILTER_SHAPES = [(3, 2, 4000, 3), (1, 1, 2, 9001), (2, 1, 257, 255)]       # (B, C, H, W): the smallest legal side of median-5, of median-3, an odd rectangle
POINTS_SHAPES = [(2, 1, 3, 5000), (1, 1, 5000, 1)]
FILL_SHAPES = [(2, 4, 40, 3000), (1, 3, 3000, 7)]
FRAME_U8_SHAPE = (3, 7, 1001)
CROP_SHAPES = [(8, 20000, 18000, 7), (20000, 6, 5, 18001), (3, 70016, 63015, 3)]      # (H, W, crop_w, crop_h)


def tiles_of(H, W):
    return -(-W // TILE_W), -(-H // TILE_H)


def scene(case, depth_to_points):
    """The cloud of a case as CPU tensors {'points' [1,3,N], 'image' [1,3,N], 'depth' [1,1,N]}: synthetic.make_rgbd, depth
    512 * 120 / (disparity + 1e-7), unprojected by `depth_to_points(depth [1,1,H,W], focal)` -- the kernel set's under test or the oracle's."""
    from ken_burns_effect_amd import synthetic
    image, disp = synthetic.make_rgbd(case.H, case.W, case.seed, case.kind)
    depth = (FOCAL * BASELINE) / (disp + 1e-7)
    points = depth_to_points(depth, FOCAL)
    return {'points': points.detach().cpu().reshape(1, 3, -1), 'image': image.reshape(1, 3, -1), 'depth': depth.reshape(1, 1, -1)}


def oracle_frame(oracle, cloud, case):
    """One frame of common.py:238-255 by the CPU oracle (Jacobi schedule: the product's), stage by stage so that every stage can be
    compared: z-buffer before and after the degrid, the un-filled render and its coverage, the filled render, the uint8 frame."""
    pts = oracle.shift_points(cloud['points'], torch.tensor(case.shift3, dtype=torch.float32))
    z0, _ = oracle.zsplat(pts, case.W, case.H, FOCAL, BASELINE)
    zd = oracle.degrid(z0, 'jacobi')
    render, existing = oracle.normalize(oracle.accumulate(pts, torch.cat([cloud['image'], cloud['depth']], 1), zd, FOCAL, BASELINE))
    filled = oracle.fill_disocclusion(render, render[:, 3:4] * (existing > 0.0).float())
    return {'z_pre': z0.numpy()[0, 0], 'z': zd.numpy()[0, 0], 'render': render.numpy()[0], 'existing': existing.numpy()[0, 0],
            'filled': filled.numpy()[0], 'frame': oracle.frame_u8(filled[0])}


def build_plan_checker(directory):
    """tests/fill_walk_check.cpp (csrc/kbe_fill_walk.h compiled by g++: the functions launch_fill runs) -> the executable's path."""
    exe = os.path.join(str(directory), 'fill_walk_check')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'ken-burns-effect_amd', 'csrc'),
                           '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'fill_walk_check.cpp'), '-o', exe])
    return exe


def fill_plans(checker, rows):
    """fill_plan of [(W, H, stages, tiles_x, tiles_y)] -> [(tables, use_strips, min_holes)]."""
    out = subprocess.run([checker, 'plan'], input=''.join('%d %d %d %d %d\n' % r for r in rows), capture_output=True, text=True, check=True)
    plans = [[int(v) for v in line.split()[:4]] for line in out.stdout.splitlines()]
    assert len(plans) == len(rows)
    return [(p[1], p[3], p[2]) for p in plans]


def fill_inputs(B, C, H, W, seed):
    """(input [B,C,H,W], depth [B,1,H,W]) of kbe_fill_disocclusion with the holes of the golden fixture's generator (tests/golden/make_golden.py:
    gen_fill) at a raster's own scale: rectangles inside, a rectangle in a corner (rays that leave the image), a slit across the whole
    short side, isolated pixels, one negative depth."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, C, H, W), dtype=np.float32)
    depth = (rng.random((B, 1, H, W), dtype=np.float32) * 900.0 + 100.0).astype(np.float32)
    long_w = W >= H
    for b in range(B):
        d = depth[b, 0]
        for _ in range(6):                                  # rectangles of up to 12 along the short side and 60 along the long one
            rh, rw = (int(rng.integers(2, min(12, H))), int(rng.integers(5, 60))) if long_w else (int(rng.integers(5, 60)), int(rng.integers(2, min(6, W))))
            y0, x0 = int(rng.integers(0, H - rh)), int(rng.integers(0, W - rw))
            d[y0:y0 + rh, x0:x0 + rw] = 0.0
        d[H - min(6, H // 2):H, 0:min(9, W // 2)] = 0.0     # touching two borders
        d[0:2, W - min(5, W // 2):W] = 0.0
        if long_w:
            d[:, W // 2] = 0.0                              # a one-pixel slit from border to border
        else:
            d[H // 2, :] = 0.0
        for _ in range(200):
            d[int(rng.integers(0, H)), int(rng.integers(0, W))] = 0.0
        d[2, min(3, W - 1)] = -1.0                          # negative depth counts as a hole too
    return torch.from_numpy(x), torch.from_numpy(depth)


def frame_u8_inputs():
    """A render [3, 7, 1001] for kbe_frame_u8 (common.py:255: clamp to [0, 1], * 255, truncate): every k / 255 with both of its fp32
    neighbours -- the values at which the truncation decides --, negatives, values above 1, both zeros and 1e30; finite throughout."""
    C, H, W = FRAME_U8_SHAPE
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    edges = np.concatenate([k, np.nextafter(k, np.float32(-1.0)), np.nextafter(k, np.float32(2.0))]).astype(np.float32)
    special = np.array([0.0, -0.0, 1e30, -1e30, -1e-30, -0.5, -3.0, 1.0000001, 1.5, 2.0, 255.0, 256.0, 1e10, 0.999999, 0.5], np.float32)
    rng = np.random.default_rng(7)
    fixed = np.concatenate([edges, special])
    rest = (rng.random(C * H * W - fixed.size, dtype=np.float32) * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
    flat = np.concatenate([fixed, rest])
    rng.shuffle(flat)
    assert np.isfinite(flat).all()
    return flat.reshape(C, H, W)
