"""Memory: every device entry of include/kbe.h under guard bands and on poisoned buffers (tests/guarded.py).

The rest of the GPU suite holds VALUES against the oracle; PyTorch's allocator hides the two things it cannot see.  Here every output and
every scratch the binding allocates is exactly the bytes the library's own size functions ask for, between two bands of sentinels that
must come back untouched, and starts out as 0x00 bytes in one run and 0xFF bytes in the next (NaN as a float, -1 as a counter, every bit
of a mask word or z key set): what the project holds bit for bit must be byte-identical between the two runs, frames within
frames_close.  So that no case passes by doing nothing, each result is also held against what the suite already uses for it -- the
oracle where an oracle test of the case exists, otherwise the same call made outside the harness -- under that test's own bar.

No bar here is new: assert_bits_equal, byte identity, frames_close (test_hip_parity.py), and for the clouds of the slow paths the bound
of the test they come from.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import elongated_cases as ec
import guarded
from conftest import assert_bits_equal
from test_hip_parity import _scene, frames_close, psnr

pytestmark = pytest.mark.gpu

F, BL = ec.FOCAL, ec.BASELINE
POISONS = (0x00, 0xFF)
CAMERA = (1.5, -0.75, -20.0)                # test_pile_up_paths' shift, at the clouds' own focal length


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def g(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def c(t):
    return t.detach().cpu().numpy()


def void(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------
# the clouds (CPU tensors: points [1,3,N], image [1,3,N], depth [1,1,N]) and the oracle's frame of each, made once and never written to
# ---------------------------------------------------------------------------------------

def _cloud(pts, img, dep):
    return {'points': pts.reshape(1, 3, -1).contiguous(), 'image': img.reshape(1, 3, -1).contiguous(), 'depth': dep.reshape(1, 1, -1).contiguous()}


@functools.lru_cache(maxsize=None)
def cloud_of(kind, H, W):
    """raster: a point per pixel (test_pipelined_groups_through_the_slow_paths' `tiny`); pile_up: 16 points per pixel (test_pile_up_paths: records
    spill, buckets overflow, the brute-force path); incoherent: random order, points at and behind the camera
    (test_degenerate_points_and_incoherent_clouds: lists abandoned, tiles scan); empty; one_tile: 40 000 points that all project into the
    first tile -- 2500 sub-blocks for a candidate list of KBE_CAND_CAP = 2048."""
    g0 = torch.Generator().manual_seed(11 + H * 131 + W)
    if kind == 'raster':
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
        z = 700.0 + 200.0 * torch.rand(H, W, generator=g0)
        pts = torch.stack([(xs - W / 2 + 0.5) * z / 512.0, (ys - H / 2 + 0.5) * z / 512.0, z])
        return _cloud(pts, torch.rand(3, H * W, generator=g0), z)
    if kind == 'pile_up':
        N = 16 * W * H
        u = torch.rand(N, generator=g0) * (W + 8) - 4 - W / 2 + 0.5
        v = torch.rand(N, generator=g0) * (H + 8) - 4 - H / 2 + 0.5
        z = torch.rand(N, generator=g0) * 400 + 600
        return _cloud(torch.stack([u * z / 512.0, v * z / 512.0, z]), torch.rand(3, N, generator=g0), z.clone())
    if kind == 'incoherent':
        N = 5000
        pts = torch.rand(1, 3, N, generator=g0) * torch.tensor([1600.0, 1200.0, 900.0]).view(1, 3, 1) - torch.tensor([800.0, 600.0, -100.0]).view(1, 3, 1)
        pts[0, 2, :50] = 0.0
        pts[0, 2, 50:100] = -30.0
        pts[0, 2, 100:120] = 0.004
        return _cloud(pts, torch.rand(3, N, generator=g0), torch.rand(N, generator=g0) * 500 + 100)
    if kind == 'empty':
        return _cloud(torch.zeros(3, 0), torch.zeros(3, 0), torch.zeros(0))
    assert kind == 'one_tile'
    N = 40000
    u = torch.rand(N, generator=g0) * (ec.TILE_W - 4) + 2 - W / 2 + 0.5         # image positions 2 .. 30 x 2 .. 14 under the unshifted camera
    v = torch.rand(N, generator=g0) * (ec.TILE_H - 4) + 2 - H / 2 + 0.5
    z = torch.rand(N, generator=g0) * 400 + 600
    return _cloud(torch.stack([u * z / 512.0, v * z / 512.0, z]), torch.rand(3, N, generator=g0), z.clone())


def camera_of(kind, H, W):
    """The camera of a case: CAMERA; the points of the single tile stay where they are; the one point of the 1x1 raster stays on its pixel."""
    return (0.0, 0.0, 0.0) if kind == 'one_tile' else ((0.2, -0.1, -20.0) if H * W == 1 else CAMERA)


@functools.lru_cache(maxsize=None)
def reference(oracle, kind, H, W):
    case = ec.FrameCase('%s %dx%d' % (kind, H, W), H, W, kind, 0, camera_of(kind, H, W), '')
    ref = ec.oracle_frame(oracle, cloud_of(kind, H, W), case)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def prepared(K, kind, H, W):
    """prepare_cloud inside a guard's block: the lanes' scratch is exactly lanes * kbe_video_scratch_stride, the packed cloud exactly kbe_cloud_pack_bytes."""
    cloud = cloud_of(kind, H, W)
    state = K.prepare_cloud(g(cloud['points']), g(cloud['image']), g(cloud['depth']), W, H)
    N = state['N']
    assert state['scratch'].numel() == state['lanes'] * int(K.lib.kbe_video_scratch_stride(W, H, N)), 'the binding adds no slack to the scratch sets'
    K._pack(state)
    assert state['packed'].numel() == int(K.lib.kbe_cloud_pack_bytes(N)), 'the binding adds no slack to the packed cloud'
    return state


def exact_set(K, gd, state):
    """ONE scratch set of exactly kbe_frame_scratch_bytes(W, H, N) bytes -- no rounding to the video loop's stride behind it --, initialised by
    kbe_frame_scratch_init, in the state's place of the lanes' sets."""
    W, H, N = state['W'], state['H'], state['N']
    scratch = gd.empty((int(K.lib.kbe_frame_scratch_bytes(W, H, N)),), torch.uint8, 'cuda')
    K._call('kbe_frame_scratch_init', void(scratch), W, H, stream())
    return dict(state, scratch=scratch, lanes=1)


def frame_outputs(gd, H, W):
    return {'render_f32': gd.empty((4, H, W), torch.float32, 'cuda'), 'existing_f32': gd.empty((H * W,), torch.float32, 'cuda'),
            'zee_f32': gd.empty((H * W,), torch.float32, 'cuda'), 'zee_pre_f32': gd.empty((H * W,), torch.float32, 'cuda')}


def assert_frame_is_the_oracles(got, ref, size, what, differ=1e-3):
    """test_frames_match_oracle's bars (`differ`: the share of uint8 values one count off; the slow-path clouds come with their own tests' share)."""
    assert_bits_equal(got['zee_pre_f32'].reshape(size), ref['z_pre'], what + ': z-buffer (pre-degrid)')
    assert_bits_equal(got['zee_f32'].reshape(size), ref['z'], what + ': z-buffer (degridded)')
    assert np.array_equal(got['existing_f32'].reshape(size) > 0, ref['existing'] > 0), what + ': same holes'
    d = np.abs(got['frame'].astype(np.int32) - ref['frame'].astype(np.int32))
    print('%s: uint8 max %d, %.2e differ' % (what, d.max() if d.size else 0, (d > 0).mean() if d.size else 0.0))
    assert d.max() <= 1 and (d > 0).mean() < differ and (d > 1).mean() < 1e-5, what


def assert_runs_agree(a, b, what):
    """Two runs of a case on buffers that started out as different bytes."""
    for key in a:
        if key == 'frame' or key == 'frames':
            frames_close(a[key], b[key], '%s: %s moves with the poison' % (what, key))
        elif key == 'existing_f32':
            assert np.array_equal(a[key] > 0, b[key] > 0), '%s: the holes move with the poison' % what
        elif key != 'render_f32':
            assert a[key].tobytes() == b[key].tobytes(), '%s: %s moves with the poison' % (what, key)


# ---------------------------------------------------------------------------------------
# 1. one frame on every route
# ---------------------------------------------------------------------------------------

# (kind, H, W, the share of values that may be one count off the oracle: frames_close's, or that of the test the cloud comes from)
FRAME_CASES = [('raster', 32, 64, 1e-3), ('raster', 17, 36, 1e-3), ('raster', 37, 50, 1e-3), ('raster', 1, 1, 1e-3), ('pile_up', 64, 96, 5e-3),
               ('incoherent', 136, 200, 2e-3), ('empty', 32, 64, 1e-3), ('one_tile', 32, 64, 5e-3)]


@pytest.mark.parametrize('route', ['fused', 'bucket'])
@pytest.mark.parametrize('kind,H,W,differ', FRAME_CASES, ids=['%s-%dx%d' % k[:3] for k in FRAME_CASES])
def test_one_frame_with_every_optional_output_writes_only_its_buffers(K, oracle, kind, H, W, differ, route):
    """kbe_render_frame_fused / kbe_render_frame_stages with render_f32, existing_f32, zee_f32 and zee_pre_f32 asked for, on the lanes' sets as
    prepare_cloud makes them, then on ONE set of exactly kbe_frame_scratch_bytes: the fused route as the frames of parity 0 and 1 -- both banks
    of lists and placements, the second of which ends the set --, the bucket route on z-buffer A and on B.  Rasters by what the code switches
    on: whole tiles and 16-byte row stores (32x64); dword stores, a partial tile column and a last tile row of one image row (17x36); an odd
    H * W, every region of the set padded (37x50); 1x1.  The 40 000 points in one tile go straight to the fused entry (the binding would
    route 19.5 points per pixel there by itself: FUSED_MAX_DENSITY)."""
    ref = reference(oracle, kind, H, W)
    cam = camera_of(kind, H, W)
    runs = []
    for poison in POISONS:
        with guarded.Guard(poison) as gd:
            state = prepared(K, kind, H, W)
            got = []
            for st, kw in [(state, {})] + [(exact_set(K, gd, state), dict(parity=p) if route == 'fused' else dict(stages=7 | (256 if p else 128))) for p in (0, 1)]:
                outs = frame_outputs(gd, H, W)
                frame = K.render_frame(st, cam, F, BL, out=gd.empty((H, W, 3), torch.uint8, 'cuda'), fused=route == 'fused', **outs, **kw)
                gd.check()
                got.append(dict({k: c(v) for k, v in outs.items()}, frame=c(frame)))
        for i, one in enumerate(got):
            what = '%s %dx%d %s, poison %#04x, %s' % (kind, H, W, route, poison, ('lane sets', 'exact set, first frame', 'exact set, second frame')[i])
            assert_frame_is_the_oracles(one, ref, (H, W), what, differ)
            assert kind == 'empty' or psnr(one['render_f32'][:3], ref['filled'][:3], 1.0) > (90.0 if kind in ('pile_up', 'one_tile') else 100.0), what
        runs.append(got)
    for a, b in zip(*runs):
        assert_runs_agree(a, b, '%s %dx%d %s' % (kind, H, W, route))


@pytest.mark.parametrize('H,W', [(32, 64), (37, 50), (1, 1)])
def test_the_generic_route_and_the_tiled_render_pointcloud_write_only_their_buffers(K, oracle, H, W):
    """KBE_FUSED=generic (kbe_shift_points, kbe_render_pointcloud, kbe_fill_disocclusion, kbe_frame_u8 per frame) into a guarded frame, and
    kbe_render_pointcloud_tiled -- whose scratch the binding sizes by kbe_frame_scratch_bytes(W, H, 0) -- at C = 4 and 7."""
    ref = reference(oracle, 'raster', H, W)
    cloud = cloud_of('raster', H, W)
    cam = camera_of('raster', H, W)
    runs = []
    for poison in POISONS:
        with guarded.Guard(poison) as gd:
            state = dict(prepared(K, 'raster', H, W), generic=True)
            out = gd.empty((1, H, W, 3), torch.uint8, 'cuda')
            K.render_video(state, [(F, cam)], BL, host_out=out)
            pts = K.shift_points(g(cloud['points']), cam)
            data = torch.cat([g(cloud['image']), g(cloud['depth']), g(cloud['image'])], 1)
            tiled = [K.render_pointcloud(pts, data[:, :C].contiguous(), W, H, F, BL, tiled=True) for C in (4, 7)]
            assert list(K._tiled_scratch.values())[0].numel() == int(K.lib.kbe_frame_scratch_bytes(W, H, 0))
        frames_close(c(out[0]), ref['frame'], 'generic route %dx%d, poison %#04x' % (H, W, poison))
        for render, existing in tiled:
            C = render.shape[1]
            assert np.array_equal(c(existing)[0, 0] > 0, ref['existing'] > 0)
            assert (np.abs(c(render)[0, :4] - ref['render']) <= 1e-4 * np.maximum(np.abs(ref['render']), 1.0)).all(), 'tiled render_pointcloud, C = %d' % C
        runs.append({'frame': c(out[0]), 'existing_f32': c(tiled[1][1])})
    assert_runs_agree(runs[0], runs[1], 'generic route %dx%d' % (H, W))


# ---------------------------------------------------------------------------------------
# 2. group launches
# ---------------------------------------------------------------------------------------

CAMERAS = [(512.0 - 6.0 * i, (1.5 * i - 4.0, 2.0 - 0.7 * i, -3.0 * i)) for i in range(19)]        # test_pipelined_groups_through_the_slow_paths'


@functools.lru_cache(maxsize=None)
def frames_on_their_own(K, H, W):
    """CAMERAS' frames of the raster cloud, one kbe_render_frame_fused each, outside the harness: what the groups are held against."""
    cloud = cloud_of('raster', H, W)
    state = K.prepare_cloud(g(cloud['points']), g(cloud['image']), g(cloud['depth']), W, H)
    alone = np.stack([c(K.render_frame(state, sh, f, BL, fused=True)) for f, sh in CAMERAS])
    alone.setflags(write=False)
    return alone


def pipelined(K, state, gd, sizes, H, W, shift=0):
    """Groups of `sizes` frames through kbe_render_frame_group_ahead, each tile launch making the next group's placements
    (test_pipelined_groups_equal_groups_with_their_placements_in_front's loop) -> the frames."""
    groups, at = [], 0
    for n in sizes:
        groups.append(CAMERAS[at:at + n])
        at += n
    turns, placed, out = [0] * 12, False, []
    for i, grp in enumerate(groups):
        n = len(grp)
        nxt = groups[i + 1] if i + 1 < len(groups) else None
        ok = nxt is not None and bool(K.lib.kbe_render_frame_group_ahead_ok(state['N'], W, H, n, len(nxt)))
        now = turns[:n]
        for k in range(n):
            turns[k] += 1
        buf = gd.empty((n, H, W, 3), torch.uint8, 'cuda', shift=shift)
        K.render_frame_group_ahead(state, grp, BL, buf, turn=now, placed=placed, next_cameras=nxt if ok else None, next_turn=turns[:len(nxt)] if ok else None)
        placed = ok
        out.append(buf)
    return torch.cat(out)


@pytest.mark.parametrize('H,W', [(37, 50), (32, 64)])
def test_group_launches_write_only_their_buffers(K, H, W):
    """kbe_render_frame_group (1 to 4 frames, z-buffers A and B), kbe_render_frame_group_fused (12 frames; five frames on sets fresh from
    kbe_frame_scratch_init_sets with parities 0, 1, 0) and kbe_render_frame_group_ahead pipelined over groups of 12, 5 and 2 frames -- both banks and both hole counters of the sets in use --
    on group scratch of exactly sets * kbe_video_scratch_stride, against the frames rendered on their own."""
    alone = frames_on_their_own(K, H, W)
    runs = []
    for poison in POISONS:
        with guarded.Guard(poison) as gd:
            state = prepared(K, 'raster', H, W)
            got = {}
            for n, flags in ((1, None), (3, [128] * 3), (4, [256] * 4), (4, None)):
                got['bucket %d %s' % (n, flags)] = K.render_frame_group(state, CAMERAS[:n], BL, gd.empty((n, H, W, 3), torch.uint8, 'cuda'), zbuf_flags=flags)
            assert state['scratch_groups'].numel() == 4 * K.scratch_stride(state)
            got['fused 12'] = K.render_frame_group_fused(state, CAMERAS[:12], BL, gd.empty((12, H, W, 3), torch.uint8, 'cuda'))
            assert state['scratch_groups'].numel() == 12 * K.scratch_stride(state) == 12 * int(K.lib.kbe_video_scratch_stride(W, H, state['N']))
            gd.check()
            # frames WITH a parity count their holes where the set's last frame left a zero: the first of them relies on what
            # kbe_frame_scratch_init_sets cleared -- hole counters and list totals --, so they run on sets of their own, fresh from it
            fresh = prepared(K, 'raster', H, W)
            for turn, parity in enumerate((0, 1, 0)):
                got['fused turn %d' % turn] = K.render_frame_group_fused(fresh, CAMERAS[:5], BL, gd.empty((5, H, W, 3), torch.uint8, 'cuda'), parities=[parity] * 5)
            assert fresh['scratch_groups'].numel() == 5 * K.scratch_stride(fresh)
            gd.check()
            got['ahead'] = pipelined(K, state, gd, [12, 5, 2], H, W)
        got = {k: c(v) for k, v in got.items()}
        for key, frames in got.items():
            frames_close(frames, alone[:len(frames)], '%dx%d %s, poison %#04x' % (H, W, key, poison))
        runs.append(got)
    for key in runs[0]:
        frames_close(runs[0][key], runs[1][key], '%dx%d %s moves with the poison' % (H, W, key))


# ---------------------------------------------------------------------------------------
# 3. the video loop
# ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def video_reference(oracle, H, W, seed, n_frames):
    """(cameras, crop, the oracle's frames, the oracle's cropped frames) of _scene((H, W), seed) on a path of n_frames steps."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((H, W), seed)
    settings = dict(settings, dblSteps=[i / (n_frames - 1) for i in range(n_frames)])
    settings.pop('boolCrop')
    cams, crop = common.frame_cameras(settings, oc), common.crop_size(settings)
    ok = oracle.OracleKernels('jacobi')
    state = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), W, H)
    frames = np.stack([ok.render_frame(state, sh, f, oc['dblBaseline']).numpy() for f, sh in cams])
    cropped = np.stack([oracle.crop_resize_u8(f, crop[0], crop[1]) for f in frames])
    for a in (frames, cropped):
        a.setflags(write=False)
    return cams, crop, frames, cropped


@pytest.mark.parametrize('fused', ['0', '1'])
@pytest.mark.parametrize('H,W', [(37, 50), (64, 96)])
def test_videos_write_only_their_buffers(K, oracle, monkeypatch, H, W, fused):
    """kbe_render_video through common.render_frames on two lanes: frames left in HBM (after a video of ANOTHER scene of the same size, dropped:
    what the allocator hands back then holds plausible stale frames), delivered to pinned memory, delivered cropped, and delivered in groups of
    four per lane.  The scratch is exactly the sets' count times kbe_video_scratch_stride and the stage exactly kbe_video_stage_bytes; the
    pinned buffers are the harness's too.  Every video against the oracle's frames of its scene."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', fused)
    monkeypatch.setenv('KBE_LANES', '2')
    monkeypatch.setenv('KBE_HOST_LANES', '2')
    n_frames = 8
    cams, crop, want, want_cropped = video_reference(oracle, H, W, 5, n_frames)
    stage_sizes = []
    ask = K.lib.kbe_video_stage_bytes
    monkeypatch.setattr(K.lib, 'kbe_video_stage_bytes', lambda *a: stage_sizes.append(int(ask(*a))) or stage_sizes[-1])
    runs = []
    for poison in POISONS:
        other = _scene((H, W), 6)[1]
        stale = common.render_frames(cams, other, None, keep_on_device=True)
        assert stale.shape == (n_frames, H, W, 3) and bool(stale.any())
        del stale, other
        with guarded.Guard(poison) as gd:
            _, oc = _scene((H, W), 5)
            got = {}
            got['in HBM'] = c(common.render_frames(cams, oc, None, keep_on_device=True, host_out=gd.empty((n_frames, H, W, 3), torch.uint8, 'cuda')))
            state = common._prepared_cloud(K, oc)
            stride = int(K.lib.kbe_video_scratch_stride(W, H, state['N']))
            assert state['lanes'] == 2 and state['scratch'].numel() == 2 * stride
            assert state['stage'].numel() == stage_sizes[-1] > 0, 'the binding adds no slack to the stage'
            got['delivered'] = common.render_frames(cams, oc, None).copy()
            got['delivered in groups'] = common.render_frames(cams, oc, None, batch=-4).copy()
            got['cropped'] = common.render_frames(cams, oc, crop).copy()
            got['cropped in HBM'] = c(common.render_frames(cams, oc, crop, keep_on_device=True, host_out=gd.empty((n_frames, H, W, 3), torch.uint8, 'cuda')))
            assert state['stage'].numel() == max(stage_sizes)
            assert 'scratch_groups' not in state or (state['scratch_groups'].numel() % stride == 0 and state['scratch_groups'].numel() >= state['video_sets'] * stride)
            assert any(a.whole.is_pinned() for a in gd.allocations), 'the delivered videos land in pinned buffers of the harness'
        for key, frames in got.items():
            what = '%dx%d fused=%s %s, poison %#04x' % (H, W, fused, key, poison)
            if 'cropped' in key:
                # (test_cropped_frames_ignore_holes_outside_the_crop's bar: the oracle fills every hole and then crops, the loop fills those the crop reads)
                d = np.abs(frames.astype(np.int32) - want_cropped.astype(np.int32))
                assert d.max() <= 2 and (d > 0).mean() < 2e-3 and (d > 1).mean() < 1e-5, '%s: max %d, %.2e differ, %.2e by more than one' % (what, d.max(), (d > 0).mean(), (d > 1).mean())
            else:
                frames_close(frames, want, what)
        runs.append(got)
    for key in runs[0]:
        frames_close(runs[0][key], runs[1][key], '%dx%d fused=%s %s moves with the poison' % (H, W, fused, key), cropped='cropped' in key)


# ---------------------------------------------------------------------------------------
# 4. the packed cloud
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [0, 1, 63, 64, 65, 4097])
def test_cloud_pack_stays_inside_kbe_cloud_pack_bytes(K, oracle, N):
    """kbe_cloud_pack into exactly kbe_cloud_pack_bytes(N) -- rocprim's temporary storage lies last in it -- followed by one fused frame at
    32x64 that reads it (z-buffers and holes against the oracle, the frame against the same call outside the harness).  65 points are the first with a second block, 64 * 64 + 1 = 4097 the first with a second node level."""
    H, W = 32, 64
    g0 = torch.Generator().manual_seed(N)
    u, v = torch.rand(N, generator=g0) * (W + 8) - 4 - W / 2 + 0.5, torch.rand(N, generator=g0) * (H + 8) - 4 - H / 2 + 0.5
    z = torch.rand(N, generator=g0) * 400 + 600
    cloud = _cloud(torch.stack([u * z / 512.0, v * z / 512.0, z]), torch.rand(3, N, generator=g0), z.clone())
    ref = ec.oracle_frame(oracle, cloud, ec.FrameCase('pack %d' % N, H, W, '', 0, CAMERA, ''))
    alone = c(K.render_frame(K.prepare_cloud(g(cloud['points']), g(cloud['image']), g(cloud['depth']), W, H), CAMERA, F, BL, fused=True))
    runs = []
    for poison in POISONS:
        with guarded.Guard(poison) as gd:
            state = K.prepare_cloud(g(cloud['points']), g(cloud['image']), g(cloud['depth']), W, H)
            assert state['fused'] and state['packed'].numel() == int(K.lib.kbe_cloud_pack_bytes(N)) and any('_pack' in a.site for a in gd.allocations)
            gd.check()
            outs = frame_outputs(gd, H, W)
            frame = K.render_frame(exact_set(K, gd, state), CAMERA, F, BL, out=gd.empty((H, W, 3), torch.uint8, 'cuda'), fused=True, **outs)
        got = dict({k: c(v) for k, v in outs.items()}, frame=c(frame))
        what = 'packed cloud of %d points, poison %#04x' % (N, poison)
        assert_bits_equal(got['zee_pre_f32'].reshape(H, W), ref['z_pre'], what + ': z-buffer (pre-degrid)')
        assert_bits_equal(got['zee_f32'].reshape(H, W), ref['z'], what + ': z-buffer (degridded)')
        assert np.array_equal(got['existing_f32'].reshape(H, W) > 0, ref['existing'] > 0), what + ': same holes'
        frames_close(got['frame'], alone, what + ': the frame of the same call outside the harness')
        runs.append(got)
    assert_runs_agree(runs[0], runs[1], 'packed cloud of %d points' % N)


# ---------------------------------------------------------------------------------------
# 5. outputs held off their allocation's start
# ---------------------------------------------------------------------------------------

SHIFTS = [0, 1, 2, 3, 4, 8]


@pytest.mark.parametrize('H,W', [(32, 64), (17, 36)])
def test_frames_held_off_their_allocations_start(K, H, W):
    """The uint8 frames of a fused group and of a bucket group in a buffer that starts 1, 2, 3, 4 and 8 bytes behind its allocation: the tile
    launches store rows as 16-byte words (32x64), as dwords (17x36's first tile column) or as bytes by the FRAME's alignment, not only the
    width's.  Both bands untouched -- the shift's bytes in front of the frames are band --, the frames those of the aligned run."""
    alone = frames_on_their_own(K, H, W)
    with guarded.Guard(0xFF) as gd:
        state = prepared(K, 'raster', H, W)
        for shift in SHIFTS:
            fused = K.render_frame_group_fused(state, CAMERAS[:3], BL, gd.empty((3, H, W, 3), torch.uint8, 'cuda', shift=shift))
            bucket = K.render_frame_group(state, CAMERAS[:3], BL, gd.empty((3, H, W, 3), torch.uint8, 'cuda', shift=shift))
            ahead = pipelined(K, state, gd, [2, 1], H, W, shift=shift)
            gd.check()
            assert fused.data_ptr() % 16 == bucket.data_ptr() % 16 == shift
            for name, frames in (('fused', fused), ('bucket', bucket), ('pipelined', ahead)):
                frames_close(c(frames), alone[:3], '%dx%d %s group %d bytes off' % (H, W, name, shift))


@pytest.mark.parametrize('H,W,cw,ch', [(32, 64, 57, 29), (17, 36, 33, 15), (37, 50, 45, 33), (48, 128, 115, 43), (1, 1, 1, 1)])
def test_crop_resize_into_an_output_held_off_its_allocations_start(K, oracle, H, W, cw, ch):
    """kbe_crop_resize_u8 (16-byte, dword and byte stores by W and by the output's alignment) through ctypes into outputs 0 to 8 bytes off:
    byte-identical to the aligned run, which is the oracle's crop."""
    frame = (np.random.default_rng(H * W).random((H, W, 3)) * 255).astype(np.uint8)
    want = oracle.crop_resize_u8(frame, cw, ch)
    src = g(frame)
    with guarded.Guard(0xFF) as gd:
        assert np.array_equal(c(K.crop_resize_u8(src, cw, ch)), want)
        for shift in SHIFTS:
            out = gd.empty((H, W, 3), torch.uint8, 'cuda', shift=shift)
            K._call('kbe_crop_resize_u8', void(src), W, H, cw, ch, void(out), stream())
            gd.check()
            assert np.array_equal(c(out), want), 'crop %dx%d -> %dx%d, %d bytes off' % (W, H, cw, ch, shift)


def test_bias_act_into_an_output_held_off_a_16_byte_boundary(K):
    """kbe_bias_act through out= on a view 4 and 8 bytes into its buffer, HW % 4 == 0: the kernel takes float4 by the pointers' alignment, so
    this runs the scalar path where the aligned call runs the vector path -- the same bits."""
    gen = torch.Generator().manual_seed(17)
    B, C, H, W = 1, 5, 12, 20
    x, r1 = torch.randn(B, C, H, W, generator=gen).cuda(), torch.randn(B, C, H, W, generator=gen).cuda()
    bias, slope = torch.randn(C, generator=gen).cuda(), (torch.rand(C, generator=gen) * 0.5 - 0.1).cuda()
    want = K.bias_act(x, bias, slope, r1)
    assert_bits_equal(c(want), c(torch.nn.functional.prelu(x + bias.view(1, -1, 1, 1), slope) + r1), 'the vector path')
    with guarded.Guard(0xFF) as gd:
        for shift in (0, 4, 8):
            out = gd.empty((B, C, H, W), torch.float32, 'cuda', shift=shift)
            assert K.bias_act(x, bias, slope, r1, out=out).data_ptr() % 16 == shift
            gd.check()
            assert_bits_equal(c(out), c(want), 'bias_act %d bytes off' % shift)


# ---------------------------------------------------------------------------------------
# 6. glue and network kernels
# ---------------------------------------------------------------------------------------

def glue_calls(K, B, C, H, W, seed=0):
    """[(name, thunk -> tensor or tuple of tensors, exact?)]: every K. wrapper of csrc/kbe_hip.hip on inputs of one shape, made once.
    seed: another set of tensors of the same shapes (tests/test_streams_gpu.py: the decoy); everything that is no tensor stays what it is."""
    gen = torch.Generator().manual_seed(B * 1000 + C * 100 + H * 10 + W + 7919 * seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    uni = lambda *s: torch.rand(*s, generator=gen).cuda()
    N = H * W
    depth = uni(B, 1, H, W) * 300 + 600
    valid = (uni(B, 1, H, W) > 0.3).float()
    x = rnd(B, C, H, W)
    points = K.depth_to_points(depth, F).view(B, 3, N).contiguous()
    shift = [3.25, -1.5, -12.0]
    moved = K.shift_points(points, shift)
    zkeys, _ = K.zsplat(moved, W, H, F, BL)
    zee = K.degrid(zkeys=zkeys)
    data4, data7 = uni(B, 4, N), uni(B, 7, N)
    acc = K.accumulate(moved, data4, zee, F, BL)
    holes = depth * (uni(B, 1, H, W) > 0.25).float()
    shifts = torch.tensor([shift, [-2.0, 1.0, 9.0]][:B]).view(B, 3, 1).cuda()
    frame = (uni(H, W, 3) * 255).to(torch.uint8)
    cw, ch = max(1, W - W // 4), max(1, H - H // 4)
    cout = C + 2
    keep = 0.3 if seed == 0 else 0.97       # (the decoy's masks are sparse, so that the windows without a valid pixel -- pconv_epilogue's second output -- are others)
    raw, mask = rnd(B, cout, H, W), (uni(B, C, H, W) > keep).float()
    bias, slope, res = rnd(cout), uni(cout) * 0.5 - 0.1, rnd(B, cout, H, W)
    slope_in, m1 = uni(C) * 0.5 - 0.1, (uni(B, 1, H, W) > keep).float()
    return [
        ('depth_to_points', lambda: K.depth_to_points(depth, F), True),
        ('depth_to_points valid', lambda: K.depth_to_points(depth, F, valid=valid), True),
        ('shift_points', lambda: K.shift_points(points, shift), True),
        ('laplacian', lambda: K.spatial_filter(x, 'laplacian'), True),
        ('median-3', lambda: K.spatial_filter(x, 'median-3'), True),
        ('median-5', lambda: K.spatial_filter(x, 'median-5'), True),
        ('laplacian_valid', lambda: K.laplacian_valid(depth, depth.max(), 0.03), True),
        ('zsplat', lambda: K.zsplat(moved, W, H, F, BL, shift3=shift, want_winner=True), True),
        ('zkeys_decode', lambda: K.zkeys_decode(zkeys), True),
        ('degrid', lambda: K.degrid(zkeys=zkeys), True),
        ('degrid from fp32', lambda: K.degrid(zee=K.zkeys_decode(zkeys)), True),
        ('degrid_serial', lambda: K.degrid_serial(zkeys=zkeys), True),
        ('accumulate', lambda: K.accumulate(moved, data4, zee, F, BL), False),
        ('normalize', lambda: K.normalize(acc), True),
        ('render_pointcloud atomic C=4', lambda: K.render_pointcloud(moved, data4, W, H, F, BL, tiled=False), False),
        ('render_pointcloud atomic C=7', lambda: K.render_pointcloud(moved, data7, W, H, F, BL, tiled=False), False),
        ('render_pointcloud tiled C=4', lambda: K.render_pointcloud(moved, data4, W, H, F, BL, tiled=True), False),
        ('render_pointcloud tiled C=7', lambda: K.render_pointcloud(moved, data7, W, H, F, BL, tiled=True), False),
        ('fill_disocclusion', lambda: K.fill_disocclusion(x, holes), True),
        ('generate_mask tables', lambda: K.generate_mask_raw(points, shifts, W, H, F, BL, want_tables=True), True),
        ('generate_mask', lambda: K.generate_mask(points, shifts, W, H, F, BL), True),
        ('frame_u8', lambda: K.frame_u8(x[:1, :1].expand(1, 3, H, W).contiguous() if C < 3 else x[:1, :3].contiguous()), True),
        ('crop_resize_u8', lambda: K.crop_resize_u8(frame, cw, ch), True),
        ('pconv_epilogue', lambda: K.pconv_epilogue(raw, bias, mask, 3, 1, 1), True),
        ('pconv_epilogue slope residual', lambda: K.pconv_epilogue(raw, bias, mask, 3, 1, 1, act_slope=slope, residual=res), True),
        ('pconv_epilogue raw_without_bias', lambda: K.pconv_epilogue(raw, bias, m1, 3, 1, 1, in_channels=C, act_slope=slope, residual=res, raw_without_bias=True), True),
        ('pconv_epilogue no mask', lambda: K.pconv_epilogue(raw, bias, None, 3, 1, 1, in_channels=C, in_size=(H, W)), True),
        ('prelu_mask', lambda: K.prelu_mask(x, slope_in, m1), True),
        ('prelu_mask no mask', lambda: K.prelu_mask(x, slope_in, None), True),
        ('bias_act', lambda: K.bias_act(raw, bias, slope, res, res), True),
        ('bias_act bare', lambda: K.bias_act(raw), True),
        ('upsample2x_act', lambda: K.upsample2x_act(x, slope_in), True),
        ('upsample2x_act bare', lambda: K.upsample2x_act(x), True),
    ]


def as_arrays(result):
    return [c(t) for t in (result if isinstance(result, tuple) else (result,)) if t is not None]


@pytest.mark.parametrize('B,C,H,W', [(2, 3, 7, 9), (1, 5, 12, 20), (1, 1, 3, 3), (1, 1, 1, 1)])
def test_glue_and_network_kernels_write_only_their_outputs(K, B, C, H, W):
    """Every K. wrapper of csrc/kbe_hip.hip at an odd shape, at a pixel count that is a multiple of four (the vector paths), at the medians'
    smallest raster and at 1x1 where the entry takes it (the medians refuse it: KbeError outside the harness as inside), every output and
    scratch of the binding exact and guarded, on 0x00 and on 0xFF: bit for bit the same call outside the harness -- which the rest of the suite
    holds against the oracle -- and, for the kernels that sum with float atomics, within test_accumulate_and_normalize's and
    test_render_pointcloud_whole's bounds with the same pixels touched."""
    from ken_burns_effect_amd import _native
    calls = glue_calls(K, B, C, H, W)
    want = {}
    for name, call, _ in calls:
        try:
            want[name] = as_arrays(call())
        except _native.KbeError as e:
            assert (H, W) == (1, 1) and 'median' in str(e), (name, e)
            want[name] = None
    assert sum(w is not None for w in want.values()) >= len(calls) - 3
    for poison in POISONS:
        for name, call, exact in calls:
            what = '%s at %s, poison %#04x' % (name, (B, C, H, W), poison)
            if want[name] is None:
                with pytest.raises(_native.KbeError):
                    call()
                continue
            with guarded.Guard(poison) as gd:
                got = as_arrays(call())
                assert gd.allocations, what + ': the wrapper allocated through the harness'
            assert len(got) == len(want[name])
            for a, b in zip(got, want[name]):
                if exact:
                    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what
                else:
                    assert np.array_equal(a == 0, b == 0), what + ': the same pixels and channels are touched'
                    assert (np.abs(a - b) <= 2e-5 * np.maximum(np.abs(b), 1.0)).all(), what
