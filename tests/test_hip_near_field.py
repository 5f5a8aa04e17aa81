"""GPU parity outside the band of the exact-arithmetic shortcuts: every splat route on the clouds of tests/near_field_cases.py against
the CPU oracle.

include/kbe.h promises the oracle's results for any finite cloud; the hot kernels keep the promise through shortcuts that hold while
dblError lies in [2^19, 1e6] -- the fp32 `c >= a + 1.0f` of the degrid and of the z test, the per-tile band decision, the division-free
dblError, the wave-uniform tests of apply_shift and project_xy -- each with a general branch behind it.  The cases leave the band at its
edge (`edge19`: a kernel on the wrong branch differs at the pixels tests/test_near_field_cases.py counts), inside a tile, in its halo
only, through negative dblError, at dblError == 1e6 (the empty key), with every regime in every wave, and on the dense z-splat.
Bars: those of tests/test_hip_parity.py at the same quantities (named at each assertion) -- none is new, none is wider."""
import numpy as np
import pytest
import torch

import near_field_cases as nf
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu
F, BL = nf.FOCAL, nf.BASELINE
LEAN, ROOMY = 1024, 2048                                    # include/kbe.h: KBE_STAGE_FUSED_LEAN / _ROOMY
FILL_MODES = (0, 8, 16, 8 | 512)                            # default, _PER_LANE, _PER_HALFWAVE, _PER_LANE | _FILL_DIST


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    kernels = _native.kernels()          # raises if libkbe_hip.so is missing: no fallback
    yield kernels
    kernels._tiled_scratch = {}


def g(a):
    return (a if torch.is_tensor(a) else nf.tensor(a)).cuda()


def c(t):
    return t.detach().cpu().numpy()


def cameras(name):
    return list(enumerate(nf.case(name).cameras))


def one_count(frame, ref, what):
    """test_random_small_scenes_against_the_oracle's bar on a frame: within one count, fewer than 5e-3 of the bytes differ."""
    d = np.abs(np.asarray(frame).astype(np.int32) - np.asarray(ref).astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3, '%s: max %d, %.2e of the bytes differ' % (what, d.max(), (d > 0).mean())


# ---------------------------------------------------------------------------------------
# the stage entries
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', nf.NAMES)
def test_stage_entries_outside_the_band(K, oracle, name):
    """kbe_zsplat (on shifted points and with shift3), kbe_degrid from keys and from fp32, kbe_degrid_serial: bit for bit.  kbe_accumulate
    + kbe_normalize under test_accumulate_and_normalize's bars, kbe_render_pointcloud under test_render_pointcloud_whole's."""
    cs = nf.case(name)
    size = (cs.H, cs.W)
    data = torch.cat([cs.image, cs.depth], 1)
    for cam, shift3 in cameras(name):
        ref = nf.oracle_frame(oracle, name, cam)
        what = '%s, camera %d' % (name, cam)
        pts = g(ref['points'])
        for keys, winner in (K.zsplat(pts, cs.W, cs.H, F, BL, want_winner=True), K.zsplat(g(cs.points), cs.W, cs.H, F, BL, shift3=shift3, want_winner=True)):
            assert_bits_equal(c(K.zkeys_decode(keys))[0, 0], ref['z_pre'], what + ': z-buffer')
            assert np.array_equal(c(winner)[0], ref['winner']), what + ': winner pixel per point'
        assert_bits_equal(c(K.degrid(zkeys=keys))[0, 0], ref['z'], what + ': degrid from keys')
        assert_bits_equal(c(K.degrid(zee=g(ref['z_pre']).reshape(1, 1, *size)))[0, 0], ref['z'], what + ': degrid from fp32')
        serial = oracle.degrid(nf.tensor(ref['z_pre']).reshape(1, 1, *size), 'serial').numpy()
        assert_bits_equal(c(K.degrid_serial(zkeys=keys)), serial, what + ': serial degrid from keys')
        assert_bits_equal(c(K.degrid_serial(zee=g(ref['z_pre']).reshape(1, 1, *size))), serial, what + ': serial degrid from fp32')
        # accumulate on the oracle's degridded z-buffer: atomic order differs from point-index order
        acc = c(K.accumulate(pts, g(data), g(ref['z']).reshape(1, 1, *size), F, BL))
        d = np.abs(acc - ref['acc']) / np.maximum(np.abs(ref['acc']), 1.0)
        print('%s: accumulate max %.2e of max(|want|, 1)' % (what, d.max()))
        assert (d <= 1e-5).all(), what
        assert np.array_equal(acc == 0, ref['acc'] == 0), what + ': exactly the same pixels / channels are touched'
        render, existing = K.normalize(g(ref['acc']))
        assert_bits_equal(c(render)[0], ref['render'], what + ': normalise')
        assert_bits_equal(c(existing)[0, 0], ref['existing'], what + ': existing')
        render, existing = K.render_pointcloud(pts, g(data), cs.W, cs.H, F, BL, tiled=False)
        assert np.array_equal(c(existing)[0, 0] > 0, ref['existing'] > 0), what + ': hole mask identical'
        assert np.abs(c(existing)[0, 0] - ref['existing']).max() <= 1e-5 * max(1.0, float(ref['existing'].max())), what
        assert (np.abs(c(render)[0] - ref['render']) <= 2e-5 * np.maximum(np.abs(ref['render']), 1.0)).all(), what


@pytest.mark.parametrize('name', nf.NAMES)
def test_tiled_render_pointcloud_outside_the_band(K, oracle, name):
    """kbe_render_pointcloud_tiled with 7 channels (a partial last chunk) under test_pile_up_paths's bars."""
    cs = nf.case(name)
    extra = torch.rand(1, 3, cs.points.shape[2], generator=torch.Generator().manual_seed(7))
    data = torch.cat([cs.image, cs.depth, extra], 1)
    for cam, _ in cameras(name):
        ref = nf.oracle_frame(oracle, name, cam)
        what = '%s, camera %d' % (name, cam)
        r_o, e_o = oracle.render_pointcloud(nf.tensor(ref['points']), data, cs.W, cs.H, F, BL, 'jacobi')
        assert_bits_equal(e_o.numpy()[0, 0], ref['existing'], what + ": the oracle's own")
        r_t, e_t = K.render_pointcloud(g(ref['points']), g(data), cs.W, cs.H, F, BL, tiled=True)
        assert np.array_equal(c(e_t) > 0, e_o.numpy() > 0), what + ': hole mask identical'
        assert np.abs(c(e_t) - e_o.numpy()).max() <= 1e-4 * float(e_o.max()), what
        assert (np.abs(c(r_t) - r_o.numpy()) <= 1e-4 * np.maximum(np.abs(r_o.numpy()), 1.0)).all(), what


# ---------------------------------------------------------------------------------------
# the frame loop: bucket route and fused route
# ---------------------------------------------------------------------------------------

def check_frame(K, oracle, name, state, fused, build=0):
    """Every camera of a case on one route, twice: with all optional outputs (the generic degrid), then with zee_f32 alone (tiles in
    the band take the fp32-only degrid).  Bars: z-buffers bit for bit (test_frames_match_oracle); `existing` and the float render
    within 1e-4 (test_pile_up_paths); the frame within one count at < 5e-3 of its bytes (the fuzz)."""
    cs = nf.case(name)
    size, hw = (cs.H, cs.W), cs.H * cs.W
    for cam, shift3 in cameras(name):
        ref = nf.oracle_frame(oracle, name, cam)
        what = '%s, camera %d, %s%s' % (name, cam, 'fused' if fused else 'bucket', {0: '', LEAN: ' lean', ROOMY: ' roomy'}[build])
        for outputs in ('all', 'zee'):
            rf = torch.empty(4, *size, device='cuda')
            ex, zd, zp = (torch.empty(hw, device='cuda') for _ in range(3))
            if outputs == 'all':
                frame = K.render_frame(state, shift3, F, BL, render_f32=rf, existing_f32=ex, zee_f32=zd, zee_pre_f32=zp, stages=7 | build, fused=fused)
                assert_bits_equal(c(zp).reshape(size), ref['z_pre'], what + ': z-buffer (pre-degrid)')
            else:
                frame = K.render_frame(state, shift3, F, BL, render_f32=rf, existing_f32=ex, zee_f32=zd, stages=7 | build, fused=fused)
            frame = c(frame).copy()
            what_o = what + ', outputs: ' + outputs
            n_bad = int((c(zd).reshape(size).view(np.uint32) != ref['z'].view(np.uint32)).sum())
            e = np.abs(c(ex).reshape(size) - ref['existing'])
            r = np.abs(c(rf) - ref['filled']) / np.maximum(np.abs(ref['filled']), 1.0)
            print('%s: degridded z-buffer differs at %d pixels; existing max %.3g (bar %.3g), off the bar at %d pixels; render max %.3g of max(1, |ref|)'
                  % (what_o, n_bad, e.max(), 1e-4 * ref['existing'].max(), (e > 1e-4 * ref['existing'].max()).sum(), r.max()))
            assert_bits_equal(c(zd).reshape(size), ref['z'], what_o + ': z-buffer (degridded)')
            assert np.array_equal(c(ex).reshape(size) > 0, ref['existing'] > 0), what_o + ': same holes'
            assert e.max() <= 1e-4 * float(ref['existing'].max()), what_o + ': existing'
            assert (r <= 1e-4).all(), what_o + ': float render'
            one_count(frame, ref['frame'], what_o)


def prepared(K, name):
    cs = nf.case(name)
    return K.prepare_cloud(g(cs.points), g(cs.image), g(cs.depth), cs.W, cs.H, raster=cs.raster)


@pytest.mark.parametrize('name', nf.NAMES)
def test_frames_outside_the_band_on_the_bucket_route(K, oracle, name):
    check_frame(K, oracle, name, prepared(K, name), fused=False)


@pytest.mark.parametrize('name', nf.NAMES)
def test_frames_outside_the_band_on_the_fused_route(K, oracle, name):
    check_frame(K, oracle, name, prepared(K, name), fused=True)


@pytest.mark.parametrize('build', [LEAN, ROOMY], ids=['lean', 'roomy'])
@pytest.mark.parametrize('name', nf.BUILD_CASES)
def test_both_builds_of_the_fused_tile_launch_at_the_edge_of_the_band(K, oracle, name, build):
    check_frame(K, oracle, name, prepared(K, name), fused=True, build=build)


@pytest.mark.parametrize('name', nf.GROUP_CASES)
def test_a_group_placed_by_the_launch_before_it_outside_the_band(K, oracle, name):
    """kbe_render_frame_group_ahead as in test_pipelined_groups_equal_groups_with_their_placements_in_front: the three cameras of a case
    as one group, twice -- the second call's placements are made by the first call's tile launch.  Both within one count of the same
    frames on their own and of the oracle's."""
    cs = nf.case(name)
    state = prepared(K, name)
    K._pack(state)
    cams = [(F, shift3) for shift3 in cs.cameras]
    n = len(cams)
    assert n == 3 and K.lib.kbe_render_frame_group_ahead_ok(state['N'], cs.W, cs.H, n, n) == 1
    alone = np.stack([c(K.render_frame(state, shift3, F, BL, fused=True)).copy() for _, shift3 in cams])
    first, second = (torch.zeros(n, cs.H, cs.W, 3, dtype=torch.uint8, device='cuda') for _ in range(2))
    K.render_frame_group_ahead(state, cams, BL, first, turn=[0] * n, placed=False, next_cameras=cams, next_turn=[1] * n)
    K.render_frame_group_ahead(state, cams, BL, second, turn=[1] * n, placed=True)
    for k in range(n):
        want = nf.oracle_frame(oracle, name, k)['frame']
        for got, call in ((first, 'placements in front'), (second, 'placed by the launch before')):
            one_count(c(got[k]), alone[k], '%s, camera %d, %s: the frame on its own' % (name, k, call))
            one_count(c(got[k]), want, "%s, camera %d, %s: the oracle's" % (name, k, call))
    assert alone.any() and not np.array_equal(alone[0], alone[1])


# ---------------------------------------------------------------------------------------
# generate_mask, the fill schedules
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', nf.MASK_CASES)
def test_generate_mask_outside_the_band(K, oracle, name):
    """kbe_generate_mask, a batch of two (the cloud and the cloud in reverse point order) under two shifts: z-buffer, owner table and
    per-point mask exact (test_generate_mask_matches_oracle_at_size)."""
    cs = nf.case(name)
    pts = torch.cat([cs.points, cs.points.flip(2)], 0).contiguous()
    shift = torch.tensor([cs.cameras[0], cs.cameras[1]], dtype=torch.float32).view(2, 3, 1)
    masks, zee, ids = K.generate_mask_raw(g(pts), g(shift), cs.W, cs.H, F, BL, want_tables=True)
    omasks, ozee, oids = oracle.generate_mask_raw(pts, shift, cs.W, cs.H, F, BL)
    assert_bits_equal(c(zee), ozee.numpy(), name + ': z-buffer')
    assert np.array_equal(c(ids), oids.numpy()), name + ': owner table'
    assert np.array_equal(c(masks), omasks.numpy()), name + ': per-point mask'
    assert 0.0 < float(omasks.mean()) < 1.0
    if name == 'far':           # a point at dblError == 1e6 never owns a pixel (the strict `zee > err` of common.py:755)
        z = pts[0, 2].numpy() + np.float32(cs.cameras[0][2])
        assert (omasks.numpy()[0, 0][nf.dbl_error(z) == nf.EMPTY] == 0).all() and (oids.numpy()[0][ozee.numpy()[0, 0] == nf.EMPTY] < 0).all()


@pytest.mark.parametrize('name', nf.FILL_CASES)
def test_hole_fill_schedules_outside_the_band(K, oracle, name):
    """One un-filled frame of the bucket route per camera through the four schedules: byte-identical to one another
    (test_hole_fill_schedules_on_the_same_unfilled_frame_are_byte_identical), within one count of the oracle's frame."""
    cs = nf.case(name)
    state = prepared(K, name)
    for cam, shift3 in cameras(name):
        ref = nf.oracle_frame(oracle, name, cam)
        unfilled = K.render_frame(state, shift3, F, BL, stages=3, fused=False).clone()
        results = []
        for mode in FILL_MODES:
            buf = unfilled.clone()
            K.render_frame(state, shift3, F, BL, out=buf, stages=4 | mode, fused=False)
            results.append(buf)
        changed = int((results[0] != unfilled).any(dim=2).sum())
        print('%s, camera %d: %d holes, %d pixels changed by the fill' % (name, cam, (ref['existing'] <= 0).sum(), changed))
        assert changed >= 16
        for mode, r in zip(FILL_MODES[1:], results[1:]):
            assert torch.equal(r, results[0]), '%s, camera %d: schedule %d against the default' % (name, cam, mode)
        one_count(c(results[0]), ref['frame'], "%s, camera %d: the oracle's frame" % (name, cam))
