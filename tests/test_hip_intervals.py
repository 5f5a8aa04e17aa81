"""Every value the device renders against its exact interval, on 8-bit images (tests/interval_cases.py has the derivation,
tests/test_interval_cases.py holds it against the CPU oracle).

The frames' older bar -- one count on fewer than 0.1 % of the bytes, a PSNR floor on the float render -- is a share and an average, and
on a flat 8-bit image two legal point orders of the reference itself miss it 35 times over.  Here nothing is a share: on the z-buffer
the suite already pins bit for bit (asserted again: the interval presupposes it)
 (a) every channel of the float render, depth included, and `existing` lie inside their intervals at every covered pixel, the covered
     set is the oracle's, an uncovered value is exactly 0;
 (b) every frame byte, filled holes included, is to_u8 of the device's own float render at that pixel;
 (c) the filled float render is oracle.fill_disocclusion of the device's own unfilled render and depth mask, bit for bit, on the
     half-wave, per-lane and table schedules;
 (d) of a video left in HBM, where only bytes come out, every byte of a covered pixel lies in its legal byte set and every hole holds the
     bytes the oracle's fill takes from the device's own frame."""
import numpy as np
import pytest
import torch

import interval_cases as ic
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu
BL = ic.BASELINE
CAMS = range(len(ic.CAMERAS))
FILL_MODES = (0, 8, 16, 8 | 512)                            # default, _PER_LANE, _PER_HALFWAVE, _PER_LANE | _FILL_DIST (include/kbe.h)
VIDEO_FRAMES = (0, 1, 2, 1, 0)                              # indices into ic.CAMERAS: five frames, the z-buffers and hole counters alternate


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    kernels = _native.kernels()          # raises if libkbe_hip.so is missing: no fallback
    yield kernels
    kernels._tiled_scratch = {}


def g(a):
    return (a if torch.is_tensor(a) else ic.tensor(a)).cuda()


def c(t):
    return t.detach().cpu().numpy()


def prepared(K, oracle, name):
    cs = ic.case(oracle, name)
    return K.prepare_cloud(g(cs.points), g(cs.image), g(cs.depth), cs.W, cs.H, raster=cs.raster)


def report(what, rv, rw=None):
    print('%s: worst |error| / tolerance %.3f%s' % (what, rv, '' if rw is None else ', weight sums %.3f' % rw))


# ---------------------------------------------------------------------------------------
# one frame on the fused and on the bucket route
# ---------------------------------------------------------------------------------------

def check_frame(K, oracle, name, fused):
    cs = ic.case(oracle, name)
    size, hw = (cs.H, cs.W), cs.H * cs.W
    state = prepared(K, oracle, name)
    for cam in CAMS:
        focal, shift3 = ic.CAMERAS[cam]
        ref = ic.exact_frame(oracle, name, cam)
        what = '%s, camera %d, %s route' % (name, cam, 'fused' if fused else 'bucket')
        rf = torch.empty(4, *size, device='cuda')
        ex, zd = (torch.empty(hw, device='cuda') for _ in range(2))
        frame = c(K.render_frame(state, shift3, focal, BL, render_f32=rf, existing_f32=ex, zee_f32=zd, fused=fused)).copy()
        rf, ex = c(rf), c(ex).reshape(size)
        assert_bits_equal(c(zd).reshape(size), ref['z'], what + ': z-buffer (degridded)')
        report(what, *ic.check_intervals(rf, ex, ref, what))                            # (a)
        assert np.array_equal(frame, ic.u8_of(rf[:3]).transpose(1, 2, 0)), what + ': a byte is not to_u8 of its float'      # (b)
        ic.check_bytes(frame, ref, what)
        unfilled = np.where(ref['covered'], rf, np.float32(0.0))                        # (c): an uncovered value is 0 before the fill
        assert_bits_equal(rf, ic.fill_of(oracle, unfilled, ex), what + ': the fill of the own unfilled render')


@pytest.mark.parametrize('name', ic.NAMES)
def test_every_value_of_a_frame_on_the_fused_route(K, oracle, name):
    check_frame(K, oracle, name, fused=True)


@pytest.mark.parametrize('name', ic.NAMES)
def test_every_value_of_a_frame_on_the_bucket_route(K, oracle, name):
    check_frame(K, oracle, name, fused=False)


@pytest.mark.parametrize('name', ic.FILL_CASES)
def test_the_in_frame_fill_is_the_oracles_fill_of_the_unfilled_render(K, oracle, name):
    """(c) through the stages interface: the bucket route's unfilled float render, `existing` and bytes (stages = 3), then each schedule
    of the fill alone (stages = 4 | mode) on copies of them."""
    cs = ic.case(oracle, name)
    size, hw = (cs.H, cs.W), cs.H * cs.W
    state = prepared(K, oracle, name)
    filled_in_all = 0
    for cam in CAMS:
        focal, shift3 = ic.CAMERAS[cam]
        ref = ic.exact_frame(oracle, name, cam)
        what = '%s, camera %d' % (name, cam)
        rf0, ex = torch.empty(4, *size, device='cuda'), torch.empty(hw, device='cuda')
        frame0 = K.render_frame(state, shift3, focal, BL, render_f32=rf0, existing_f32=ex, stages=3, fused=False).clone()
        unfilled, existing = c(rf0), c(ex).reshape(size)
        report(what + ', unfilled', *ic.check_intervals(unfilled, existing, ref, what))
        assert (unfilled[:, ~ref['covered']] == 0).all(), what + ': an uncovered value is exactly 0'
        assert np.array_equal(c(frame0), ic.u8_of(unfilled[:3]).transpose(1, 2, 0)), what + ': unfilled bytes'
        want = ic.fill_of(oracle, unfilled, existing)
        filled_in_all += int((want != unfilled).any(0).sum())
        for mode in FILL_MODES:
            rf, frame = rf0.clone(), frame0.clone()
            K.render_frame(state, shift3, focal, BL, render_f32=rf, out=frame, stages=4 | mode, fused=False)
            assert_bits_equal(c(rf), want, '%s, schedule %d: the filled float render' % (what, mode))
            assert np.array_equal(c(frame), ic.u8_of(want[:3]).transpose(1, 2, 0)), '%s, schedule %d: filled bytes' % (what, mode)
    assert filled_in_all >= 8


# ---------------------------------------------------------------------------------------
# kbe_render_pointcloud: the atomic stages, the tile renderer at 4 and 7 channels
# ---------------------------------------------------------------------------------------

def extra_channels(n):
    return ic.colours_u8(np.random.default_rng(7).integers(0, 256, (3, n), dtype=np.uint8))


@pytest.mark.parametrize('name', ic.NAMES)
def test_every_value_of_render_pointcloud(K, oracle, name):
    cs = ic.case(oracle, name)
    extra = extra_channels(cs.points.shape[2])
    data4, data7 = ic.data_of(cs), torch.cat([ic.data_of(cs), extra], 1)
    for cam in CAMS:
        focal, _ = ic.CAMERAS[cam]
        ref, ref7 = ic.exact_frame(oracle, name, cam), ic.exact_frame(oracle, name, cam, extra)
        assert np.array_equal(ref7['n'], ref['n'])
        pts = g(ref['points'])
        for route, data, r, tiled in (('atomic stages', data4, ref, False), ('tiled, 4 channels', data4, ref, True), ('tiled, 7 channels', data7, ref7, True)):
            what = '%s, camera %d, %s' % (name, cam, route)
            render, existing = K.render_pointcloud(pts, g(data), cs.W, cs.H, focal, BL, tiled=tiled)
            render, existing = c(render)[0], c(existing)[0, 0]
            report(what, *ic.check_intervals(render, existing, r, what))
            assert (render[:, ~r['covered']] == 0).all(), what + ': an uncovered value is exactly 0'


# ---------------------------------------------------------------------------------------
# videos left in HBM: only bytes come out
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ['fused', 'bucket'])
@pytest.mark.parametrize('name', ic.VIDEO_CASES)
def test_every_byte_of_a_video_in_hbm(K, oracle, monkeypatch, name, route):
    """(d): five frames on two lanes.  A hole holds the bytes that the oracle's fill, run on the device's own frame under the oracle's
    hole mask and the exact depth, copies there (tests/test_interval_cases.py: no choice of that fill hangs on the depth's last bits) --
    so a covered pixel taken for a hole, or a hole left alone, shows."""
    monkeypatch.setenv('KBE_FUSED', '1' if route == 'fused' else '0')
    monkeypatch.setenv('KBE_LANES', '2')
    cs = ic.case(oracle, name)
    state = prepared(K, oracle, name)
    assert state['lanes'] == 2 and state['fused'] == (route == 'fused')
    out = torch.zeros(len(VIDEO_FRAMES), cs.H, cs.W, 3, dtype=torch.uint8, device='cuda')
    K.render_video(state, [ic.CAMERAS[k] for k in VIDEO_FRAMES], BL, host_out=out)
    torch.cuda.synchronize()
    frames = c(out)
    for i, cam in enumerate(VIDEO_FRAMES):
        ref = ic.exact_frame(oracle, name, cam)
        what = '%s, %s route, frame %d (camera %d)' % (name, route, i, cam)
        ic.check_bytes(frames[i], ref, what)
        want = ic.filled_bytes(oracle, frames[i], ref)
        assert np.array_equal(frames[i], want), '%s: %d hole pixels differ from the fill of the own frame' % (what, (frames[i] != want).any(2).sum())
