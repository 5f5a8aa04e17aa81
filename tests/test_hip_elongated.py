"""GPU parity on rasters far from square: every code path that ONE side of the raster selects, against the CPU oracle.

The shapes and what each crosses are tests/elongated_cases.py's: more than 512 tile columns / tile rows (the strip tables of the
table-driven hole fill are left out), the 11 000-pixel limit of those tables from either side, a single partial tile row with a width
beyond the packed cloud's Morton clamp, k_degrid_serial's loop over more rows than its workgroup has threads, and the glue kernels
(filters, unprojection, fill, uint8, crop) with many workgroups on rasters whose short side is the smallest they take.  Bars: those of
tests/test_hip_parity.py (test_frames_match_oracle, test_torch_glue_bit_exact, frames_close) -- none is wider here.

Every test that allocates scratch first asserts, from kbe_frame_scratch_bytes and the sizes of its own tensors, that it stays below
1 GB of device memory; each frame-loop state is made with KBE_LANES=1 (one scratch set) unless the test is about two lanes."""
import numpy as np
import pytest
import torch

import elongated_cases as ec
from conftest import assert_bits_equal
from test_hip_parity import frames_close, psnr

pytestmark = pytest.mark.gpu
F, BL = ec.FOCAL, ec.BASELINE


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    kernels = _native.kernels()          # raises if libkbe_hip.so is missing: no fallback
    yield kernels
    kernels._tiled_scratch = {}          # (the tiled render_pointcloud keeps its last scratch: 280 MB at 5 x 70016)


@pytest.fixture(scope='module')
def plan_checker(tmp_path_factory):
    return ec.build_plan_checker(tmp_path_factory.mktemp('fill_walk'))


def g(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def c(t):
    return t.detach().cpu().numpy()


_CLOUDS, _REFS = {}, {}


def cloud_of(K, name):
    """The case's cloud (CPU tensors), made once per raster and scene: the frames, the fills, the groups and the videos share theirs."""
    case = ec.FRAME[name]
    key = (case.H, case.W, case.kind, case.seed)
    if key not in _CLOUDS:
        _CLOUDS[key] = ec.scene(case, lambda depth, focal: K.depth_to_points(depth.cuda(), focal))
    return _CLOUDS[key]


def reference(K, oracle, name):
    """The oracle's frame of a case, rendered once and shared (never written to)."""
    if name not in _REFS:
        ref = ec.oracle_frame(oracle, cloud_of(K, name), ec.FRAME[name])
        for a in ref.values():
            a.setflags(write=False)
        _REFS[name] = ref
    return _REFS[name]


def prepared(K, name, monkeypatch, lanes=1, extra_bytes=0):
    """prepare_cloud of a case on `lanes` scratch sets, after the assertion that the test's device memory stays under the budget:
    the sets, the packed cloud, the cloud itself, and `extra_bytes` for what the test allocates besides."""
    case = ec.FRAME[name]
    cloud = cloud_of(K, name)
    n = cloud['points'].shape[2]
    need = lanes * int(K.lib.kbe_video_scratch_stride(case.W, case.H, n)) + int(K.lib.kbe_cloud_pack_bytes(n)) + 28 * n + 3 * n + extra_bytes
    assert int(K.lib.kbe_frame_scratch_bytes(case.W, case.H, n)) > 0 and need < ec.DEVICE_BUDGET, '%s: %.0f MB of device memory' % (name, need / 1e6)
    print('%s: device memory %.0f MB' % (name, need / 1e6))
    monkeypatch.setenv('KBE_LANES', str(lanes))
    state = K.prepare_cloud(g(cloud['points']), g(cloud['image']), g(cloud['depth']), case.W, case.H)
    assert state['lanes'] == lanes and state['fused'] and (state['raster_w'], state['raster_n']) == (case.W, n)
    return case, state


# ---------------------------------------------------------------------------------------
# A. the frame loop, three routes, against the oracle
# ---------------------------------------------------------------------------------------

def test_the_cases_cross_what_they_are_there_for(K, oracle):
    """The path preconditions of section A, from the oracle's frames: tile counts, holes, rows / columns that are all holes."""
    tiles = {name: ec.tiles_of(ec.FRAME[name].H, ec.FRAME[name].W) for name in ec.FRAME}
    assert tiles['48x16416'] == (513, 3) and tiles['8208x40'] == (2, 513) and tiles['8192x40'] == (2, 512)
    assert tiles['5x70016_in'] == (2188, 1) and tiles['11000x33'] == (2, 688) and tiles['11001x33'] == (2, 688)
    assert 40 % ec.TILE_W and 33 % ec.TILE_W and 5 < ec.TILE_H and 70016 > ec.MORTON_CLAMP_W
    assert ec.FRAME['11000x33'].H == ec.TABLES_MAX_SIDE and ec.FRAME['11001x33'].H == ec.TABLES_MAX_SIDE + 1
    holes = {name: reference(K, oracle, name)['existing'] <= 0 for name in ec.ORACLE_CASES}
    for name in ec.ORACLE_CASES:
        print('%s: tiles %s, %d holes, %d rows and %d columns all holes' % (name, tiles[name], holes[name].sum(), holes[name].all(axis=1).sum(), holes[name].all(axis=0).sum()))
        assert holes[name].sum() > 100, name
    assert holes['8208x40'].sum() > 20000 and holes['8208x40'].all(axis=1).sum() > 100
    assert holes['5x70016_in'].all(axis=0).sum() > 500 and holes['5x70016_in'].all(axis=1).sum() == 0 and holes['5x70016_out'].all(axis=1).sum() == 0


@pytest.mark.parametrize('name', ec.ORACLE_CASES)
def test_elongated_frames_match_the_oracle_on_all_three_routes(K, oracle, name, monkeypatch):
    """Bucket route, fused route and the tiled render_pointcloud (the scatter alone) under the bars of test_frames_match_oracle:
    z-buffer before and after the degrid bit for bit, the same holes, the float render beyond 100 dB, the uint8 frame within one
    count at fewer than 1e-3 of its values."""
    ref = reference(K, oracle, name)
    case0 = ec.FRAME[name]
    size = (case0.H, case0.W)
    hw = case0.H * case0.W
    case, state = prepared(K, name, monkeypatch, extra_bytes=int(K.lib.kbe_frame_scratch_bytes(case0.W, case0.H, 0)) + 4 * hw * 20)
    cloud = cloud_of(K, name)
    src = (cloud['image'].reshape(3, *size).permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    for fused in (False, True):
        what = '%s %s' % (name, 'fused' if fused else 'bucket')
        rf = torch.empty(4, *size, device='cuda')
        ex, zd, zp = (torch.empty(hw, device='cuda') for _ in range(3))
        frame = c(K.render_frame(state, case.shift3, F, BL, render_f32=rf, existing_f32=ex, zee_f32=zd, zee_pre_f32=zp, fused=fused))
        assert_bits_equal(c(zp).reshape(size), ref['z_pre'], what + ': z-buffer (pre-degrid)')
        assert_bits_equal(c(zd).reshape(size), ref['z'], what + ': z-buffer (degridded)')
        assert np.array_equal(c(ex).reshape(size) > 0, ref['existing'] > 0), what + ': same holes'
        p = psnr(c(rf)[:3], ref['filled'][:3], 1.0)
        d = np.abs(frame.astype(np.int32) - ref['frame'].astype(np.int32))
        print('%s: float render %.1f dB, uint8 max %d, %.2e differ' % (what, p, d.max(), (d > 0).mean()))
        assert p > 100.0, what
        frames_close(frame, ref['frame'], what)
        assert abs(psnr(frame, src, 255.0) - psnr(ref['frame'], src, 255.0)) < 1e-3, what
        again = c(K.render_frame(state, case.shift3, F, BL, fused=fused))          # without the debug outputs
        frames_close(again, frame, what + ': debug outputs do not change the frame')
    # the scatter alone, through the tile machinery, on the shifted points
    pts = K.shift_points(g(cloud['points']), case.shift3)
    data = torch.cat([g(cloud['image']), g(cloud['depth'])], 1)
    render, existing = K.render_pointcloud(pts, data, case.W, case.H, F, BL, tiled=True)
    assert np.array_equal(c(existing)[0, 0] > 0, ref['existing'] > 0), name + ' tiled render_pointcloud: same pixels covered'
    assert psnr(c(render)[0, :3], ref['render'][:3], 1.0) > 100.0
    assert (np.abs(c(render)[0] - ref['render']) <= 1e-4 * np.maximum(np.abs(ref['render']), 1.0)).all(), name + ' tiled render_pointcloud: all four channels'


# ---------------------------------------------------------------------------------------
# B. the hole-fill schedules on those shapes
# ---------------------------------------------------------------------------------------

def test_fill_plans_of_the_elongated_shapes(plan_checker):
    """The precondition of the test below, from the functions launch_fill runs (csrc/kbe_fill_walk.h, compiled by g++): which of the shapes
    fill with the tables, and with or without their strips -- so that a later change of a threshold cannot quietly empty that test."""
    names = sorted(ec.FILL_CASES)
    rows = [(ec.FRAME[n].W, ec.FRAME[n].H, 4 | ec.PER_LANE | ec.DIST) + ec.tiles_of(ec.FRAME[n].H, ec.FRAME[n].W) for n in names]
    for name, (tables, strips, min_holes) in zip(names, ec.fill_plans(plan_checker, rows)):
        want_tables, want_strips = ec.FILL_CASES[name]
        print('%s: tables %d, use_strips %d, min_holes %d' % (name, tables, strips, min_holes))
        assert tables == want_tables and min_holes == 0, name
        assert want_strips is None or strips == want_strips, name
    # ... and none of the other schedules uses them
    others = [r[:2] + (4 | mode,) + r[3:] for r in rows for mode in (0, ec.PER_LANE, ec.PER_HALFWAVE)]
    assert all(p[0] == 0 for p in ec.fill_plans(plan_checker, others))


@pytest.mark.parametrize('name', sorted(ec.FILL_CASES))
def test_hole_fill_schedules_on_elongated_frames_are_byte_identical_and_the_oracles(K, oracle, name, monkeypatch):
    """One un-filled frame of the bucket route through the four schedules (a fill never reads a hole, so it can be repeated on copies):
    byte-identical to one another; byte-identical to the ORACLE's fill of that very un-filled render (the fill copies a pixel: which
    one is all it decides, and uint8 of a copy is the copy of the uint8); and within the accumulation order (frames_close) of the
    oracle's own frame, whose un-filled render differs from the device's in the last place of its sums."""
    case0 = ec.FRAME[name]
    size, hw = (case0.H, case0.W), case0.H * case0.W
    case, state = prepared(K, name, monkeypatch, extra_bytes=4 * hw * 6 + 3 * hw * 6)
    rf = torch.empty(4, *size, device='cuda')
    ex = torch.empty(hw, device='cuda')
    unfilled = K.render_frame(state, case.shift3, F, BL, render_f32=rf, existing_f32=ex, stages=3, fused=False).clone()
    results = []
    for mode in ec.FILL_MODES:
        buf = unfilled.clone()
        K.render_frame(state, case.shift3, F, BL, out=buf, stages=4 | mode, fused=False)
        results.append(buf)
    n_holes = int((ex <= 0).sum())
    changed = int((results[0] != unfilled).any(dim=2).sum())
    print('%s: %d holes, %d pixels changed by the fill' % (name, n_holes, changed))
    # (on a raster 40 pixels wide most rays leave the image before both ends stand on valid pixels: such holes stay as they are, as in
    # the reference -- how many is the oracle's to say, below; here: the fill has thousands of holes to decide)
    assert n_holes > 1000 and changed > 1000
    for mode, r in zip(ec.FILL_MODES[1:], results[1:]):
        assert torch.equal(r, results[0]), '%s: schedule %d against the default' % (name, mode)
    render = rf.cpu()[None]
    depth = render[:, 3:4] * (ex.cpu().reshape(1, 1, *size) > 0.0).float()
    want = oracle.frame_u8(oracle.fill_disocclusion(render, depth)[0])
    assert np.array_equal(c(results[0]), want), name + ": the oracle's fill of the same un-filled render"
    frames_close(c(results[0]), reference(K, oracle, name)['frame'], name + ": the oracle's frame")


# ---------------------------------------------------------------------------------------
# C. groups of frames, a delivered video
# ---------------------------------------------------------------------------------------

def _cameras(case, n):
    """n cameras around the case's own: focal and shift change a little from frame to frame."""
    return [(F * (1.0 + 0.003 * i), tuple(float(v) * (1.0 - 0.08 * i) for v in case.shift3)) for i in range(n)]


@pytest.mark.parametrize('name', ec.GROUP_CASES)
def test_a_fused_group_on_an_elongated_raster_equals_its_frames_on_their_own(K, name, monkeypatch):
    case0 = ec.FRAME[name]
    n = case0.H * case0.W
    stride = int(K.lib.kbe_video_scratch_stride(case0.W, case0.H, n))
    case, state = prepared(K, name, monkeypatch, extra_bytes=3 * stride + 3 * n * 8)
    cams = _cameras(case, 3)
    K.group_scratch(state, 3)                           # three sets, not the four of a first use: 4 x 218 MB + the lane's is past the budget at 48 x 16416
    assert state['scratch_groups'].numel() == 3 * stride
    alone = torch.stack([K.render_frame(state, sh, f, BL).clone() for f, sh in cams])
    out = torch.zeros(3, case.H, case.W, 3, dtype=torch.uint8, device='cuda')
    K.render_frame_group_fused(state, cams, BL, out, stages=6)
    assert state['scratch_groups'].numel() == 3 * stride
    frames_close(c(out), c(alone), name + ': three frames per launch')
    assert float((alone == 0).all(dim=3).float().mean()) < 0.2, 'frames are rendered'
    assert not torch.equal(alone[0], alone[2]), 'the cameras differ'


@pytest.mark.parametrize('name', ec.GROUP_CASES)
def test_a_cropped_video_on_an_elongated_raster_equals_its_frames_cropped_one_by_one(K, name, monkeypatch):
    """kbe_render_video, five frames on two lanes, cropped, left on the device."""
    from ken_burns_effect_amd import common
    case0 = ec.FRAME[name]
    n = case0.H * case0.W
    monkeypatch.setenv('KBE_FILL_GROUP', '1')           # one frame per launch: the video renders on the lanes' own two sets
    stage = int(K.lib.kbe_video_stage_bytes(case0.W, case0.H, 2, 0))
    case, state = prepared(K, name, monkeypatch, lanes=2, extra_bytes=stage + 3 * n * 12)
    cams = _cameras(case, 5)
    cw, ch = ec.CROPS[name]
    out = torch.zeros(5, case.H, case.W, 3, dtype=torch.uint8, device='cuda')
    K.render_video(state, cams, BL, crop=(cw, ch), host_out=out)
    torch.cuda.synchronize()
    assert 'scratch_groups' not in state and state['video_sets'] == 2
    rect = common.crop_window(case.W, case.H, cw, ch)
    want = torch.stack([K.crop_resize_u8(K.render_frame(state, sh, f, BL, fill_rect=rect), cw, ch) for f, sh in cams])
    frames_close(c(out), c(want), name + ': cropped video', cropped=True)
    assert float((want == 0).all(dim=3).float().mean()) < 0.2, 'frames are rendered'


# ---------------------------------------------------------------------------------------
# D. kbe_degrid_serial past the threads of its workgroup
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', ec.DEGRID_SERIAL_SHAPES, ids=lambda s: '%dx%d' % s)
def test_serial_degrid_with_more_rows_than_threads_equals_the_oracle(K, oracle, shape):
    """White-noise depth as in test_serial_degrid_entry_at_size_equals_the_oracle, batch 2, H > 1024: every front of the wavefront takes
    the loop `y += blockDim.x` more than once."""
    H, W = shape
    rng = np.random.default_rng(5)
    zee = (1e6 - 61440.0 / (rng.random((2, 1, H, W)) * 900 + 100)).astype(np.float32)
    zee[rng.random(zee.shape) < 0.1] = 1e6
    ser = oracle.degrid(torch.from_numpy(zee), 'serial').numpy()
    share = float((ser != oracle.degrid(torch.from_numpy(zee), 'jacobi').numpy()).mean())
    print('%d x %d: serial != jacobi in %.1f %% of the pixels' % (H, W, 100 * share))
    assert H > 1024 and share > 0.05
    assert_bits_equal(c(K.degrid_serial(zee=g(zee))), ser, 'serial degrid, %d rows' % H)


# ---------------------------------------------------------------------------------------
# E. the glue kernels beyond their fixtures, bit for bit
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', ec.FILTER_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_filters_on_elongated_planes_bit_exact(K, oracle, shape):
    from ken_burns_effect_amd._native import KbeError
    B, C, H, W = shape
    rng = np.random.default_rng(H + W)
    x = (rng.random(shape, dtype=np.float32) * 100.0).astype(np.float32)
    x[rng.random(shape) < 0.2] = 0.0                                            # ties for the medians
    for kind, side in (('median-3', 2), ('median-5', 3), ('laplacian', 1)):
        if min(H, W) < side:                                                    # (reflect pad: refused, as the reference's F.pad does)
            with pytest.raises(KbeError):
                K.spatial_filter(g(x), kind)
            continue
        assert_bits_equal(c(K.spatial_filter(g(x), kind)), oracle.spatial_filter(torch.from_numpy(x), kind).numpy(), '%s %s' % (kind, shape))
    disp = g(x)
    valid = c(K.laplacian_valid(disp, disp.max(), 0.03))
    x0 = torch.from_numpy(x)
    want = (oracle.spatial_filter(x0 / x0.max(), 'laplacian').abs() < 0.03).float().numpy()
    assert_bits_equal(valid, want, 'laplacian_valid %s' % (shape,))
    assert 0.0 < want.mean() < 1.0, 'both answers occur'


@pytest.mark.parametrize('shape', ec.POINTS_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_depth_to_points_on_elongated_planes_bit_exact(K, oracle, shape):
    rng = np.random.default_rng(shape[3])
    depth = (rng.random(shape, dtype=np.float32) * 5000.0 + 100.0).astype(np.float32)
    valid = (rng.random(shape) < 0.7).astype(np.float32)
    for focal in (512.0, 153.60000000000002):
        assert_bits_equal(c(K.depth_to_points(g(depth), focal)), oracle.depth_to_points(torch.from_numpy(depth), focal).numpy(), 'depth_to_points %s' % (shape,))
        want = oracle.OracleKernels().depth_to_points(torch.from_numpy(depth), focal, valid=torch.from_numpy(valid)).numpy()
        assert_bits_equal(c(K.depth_to_points(g(depth), focal, valid=g(valid))), want, 'depth_to_points with valid %s' % (shape,))


@pytest.mark.parametrize('shape', ec.FILL_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_fill_disocclusion_on_elongated_planes_bit_exact(K, oracle, shape):
    x, depth = ec.fill_inputs(*shape, seed=shape[2])
    holes = (depth <= 0).sum().item()
    assert holes > 500 and (depth < 0).sum().item() == shape[0]
    want = oracle.fill_disocclusion(x, depth).numpy()
    assert (want != x.numpy()).any(axis=1).sum() > 0.5 * holes, 'the holes are filled'
    assert_bits_equal(c(K.fill_disocclusion(g(x), g(depth))), want, 'fill %s' % (shape,))


def test_frame_u8_against_the_oracle_at_every_boundary(K, oracle):
    x = ec.frame_u8_inputs()
    want = oracle.frame_u8(torch.from_numpy(x))
    assert set(np.unique(want).tolist()) == set(range(256))
    got = c(K.frame_u8(g(x)[None]))
    assert got.shape == want.shape == (7, 1001, 3) and np.array_equal(got, want), '%d values differ' % int((got != want).sum())


@pytest.mark.parametrize('shape', ec.CROP_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_crop_resize_on_elongated_frames_byte_exact(K, oracle, shape):
    H, W, cw, ch = shape
    f = (np.random.default_rng(W).random((H, W, 3)) * 255).astype(np.uint8)
    assert np.array_equal(c(K.crop_resize_u8(g(f), cw, ch)), oracle.crop_resize_u8(f, cw, ch))
