"""Host logic of ken_burns_effect_amd.common (camera path, point-cloud growth, frame loop) on CPU.

The kernel set is substituted EXPLICITLY with the oracle here (tests only); the product has no
CPU path.  Golden traces come from the reference's process_kenburns (serial degrid schedule,
pre-crop frames because the generator's cv2 stand-ins were identities).
"""
import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, at_size_scene, load_golden, psnr_u8


@pytest.fixture()
def common(oracle, monkeypatch):
    from ken_burns_effect_amd import common as C
    monkeypatch.setattr(C, '_kernel_set', oracle.OracleKernels(schedule='serial'))
    return C


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _depthrange(v):
    return (float(v[0]), float(v[1]), (int(v[2]), int(v[3])), (int(v[4]), int(v[5])))


def _scene(z):
    from ken_burns_effect_amd import synthetic
    image, disp = _t(z['image']), _t(z['disparity'])
    H, W = image.shape[2:]
    depth = (512.0 * 120) / (disp + 1e-7)
    from oracle import kbe_oracle
    pts = kbe_oracle.depth_to_points(depth, 512.0)
    common = {'dblFocal': 512.0, 'dblBaseline': 120, 'intWidth': W, 'intHeight': H,
              'dblDispmin': disp.min().item(), 'dblDispmax': disp.max().item(),
              'objectDepthrange': _depthrange(z['depthrange']), 'tensorRawPoints': pts.view(1, 3, -1),
              'tensorRawImage': image, 'tensorRawDisparity': disp, 'tensorRawDepth': depth}
    assert synthetic.depthrange_of(depth) == common['objectDepthrange']
    ofrom, oto = synthetic.default_windows(H, W, bool(z['dolly']))
    settings = {'dblSteps': [float(s) for s in z['steps']], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': True,
                'dolly': bool(z['dolly']), 'boolCrop': False}
    return settings, common


class ReplayInpaint:
    """Returns what the reference's Inpaint returned for the same call (recorded in the fixture)."""

    def __init__(self, z):
        self.z, self.i, self.shifts = z, 0, []

    def pointcloud_inpainting(self, tensorImage, tensorDisparity, tensorShift, objectCommon, dblFocal=None):
        out = {k: _t(self.z['inpaint%d_%s' % (self.i, k)]) for k in ('tensorExisting', 'tensorImage', 'tensorDisparity')}
        self.i += 1
        self.shifts.append(tensorShift.clone())
        return out


def test_process_shift_matches_reference(common):
    z = load_golden('torch_helpers')
    oc = {'dblFocal': 512.0, 'intWidth': 32, 'intHeight': 24, 'objectDepthrange': _depthrange(z['ps_depthrange'])}
    pts = _t(z['ps_points'])
    for i, (su, sv, ratio, focal) in enumerate(z['ps_settings']):
        st = {'tensorPoints': pts, 'dblShiftU': float(su), 'dblShiftV': float(sv), 'dblDepthFrom': oc['objectDepthrange'][0],
              'dblDepthTo': oc['objectDepthrange'][0] * float(ratio)}
        out, shift = common.process_shift(st, oc) if focal < 0 else common.process_shift(st, oc, float(focal))
        assert_bits_equal(shift.numpy(), z['ps_shift_%d' % i], 'tensorShift')
        assert_bits_equal(out.numpy(), z['ps_out_%d' % i], 'shifted points')
    assert_bits_equal(pts.numpy(), z['ps_points'], 'inputs are never mutated')


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_process_autozoom_matches_the_reference_run(common, tag):
    """common.py:114-170.  The reference's process_autozoom is dead code that cannot run as written (it calls process_shift without
    objectCommon, :146-152); the fixture holds what its unmodified body returns once that one argument is supplied
    (tests/golden/make_golden.py: gen_autozoom): the crop window, out of a 16 x 16 grid of shifts, under which the shifted cloud
    covers the most pixels -- this package's version must pick the same window (test it or delete it)."""
    from oracle import kbe_oracle
    z = load_golden('autozoom')
    image, disp = _t(z[tag + '_image']), _t(z[tag + '_disparity'])
    H, W = image.shape[2:]
    depth = (512.0 * 120) / (disp + 1e-7)
    oc = {'dblFocal': 512.0, 'dblBaseline': 120, 'intWidth': W, 'intHeight': H, 'objectDepthrange': _depthrange(z[tag + '_depthrange']),
          'tensorRawPoints': kbe_oracle.depth_to_points(depth, 512.0).view(1, 3, -1), 'tensorRawImage': image, 'tensorRawDisparity': disp, 'tensorRawDepth': depth}
    settings = {'dblShift': float(z[tag + '_shift']), 'dblZoom': float(z[tag + '_zoom']),
                'objectFrom': {'dblCenterU': W / 2.0, 'dblCenterV': H / 2.0, 'intCropWidth': W, 'intCropHeight': H}}
    got = common.process_autozoom(settings, oc)
    want = z[tag + '_window']
    assert [got['dblCenterU'], got['dblCenterV'], got['intCropWidth'], got['intCropHeight']] == [float(want[0]), float(want[1]), int(want[2]), int(want[3])]
    assert isinstance(got['intCropWidth'], int) and isinstance(got['intCropHeight'], int)


def test_dolly_trace_matches_reference(common):
    z = load_golden('kenburns_dolly')
    settings, oc = _scene(z)
    frames = common.process_kenburns(settings, oc, None)
    assert len(frames) == len(z['frames'])
    for f, g in zip(frames, z['frames']):
        assert f.dtype == np.uint8 and np.array_equal(f, g)
    assert oc['tensorInpaPoints'].shape[2] == z['inpa_points'].shape[2]    # dolly never inpaints (common.py:217)


def test_kenburns_trace_matches_reference(common):
    z = load_golden('kenburns_kbe')
    settings, oc = _scene(z)
    frames = common.process_kenburns(settings, oc, ReplayInpaint(z))
    for key, name in (('tensorInpaPoints', 'inpa_points'), ('tensorInpaImage', 'inpa_image'),
                      ('tensorInpaDepth', 'inpa_depth'), ('tensorInpaDisparity', 'inpa_disparity')):
        assert_bits_equal(oc[key].numpy(), z[name], key)
    for f, g in zip(frames, z['frames']):
        assert np.array_equal(f, g)


def test_jacobi_schedule_stays_close_to_serial(oracle, monkeypatch):
    """The normative (out-of-place) degrid differs from the serial reference schedule only slightly;
    the gap is reported, not hidden."""
    from ken_burns_effect_amd import common as C
    z = load_golden('kenburns_dolly')
    monkeypatch.setattr(C, '_kernel_set', oracle.OracleKernels(schedule='jacobi'))
    settings, oc = _scene(z)
    frames = C.process_kenburns(settings, oc, None)
    # These 40x56 scenes carry full-size disparity ranges (steep per-pixel depth steps) and white-noise
    # colours, so they are far more degrid-sensitive than a real image: ~5-9 % of the uint8 values move.
    # Both schedules are legal outcomes of the reference's racy in-place kernel (common.py:556-566).
    diff = np.mean([np.mean(f != g) for f, g in zip(frames, z['frames'])])
    assert 0.0 < diff < 0.25


# PSNR floors of the product's (Jacobi) schedule against the reference-run frames; measured on the CPU oracle: noise colours KBE
# 32.2-36.1 dB, dolly 33.9-43.5; photograph-like colours (synthetic.photo_like) KBE 44.2-51.6 dB (0.10-0.34 % of the pixels moved
# by more than a count, by up to 153: pixels that one schedule leaves to the SEEDED-RANDOM Inpaint network's colours and the
# other to the surface -- a trained network's colours would blend in), dolly 50.2-59.0 dB (no network there, moves of <= 70)
JACOBI_FLOOR_DB = {'kbe': 30.0, 'dolly': 30.0, 'kbe_photo': 43.0, 'dolly_photo': 49.0}


@pytest.mark.parametrize('tag', ['kbe', 'dolly', 'kbe_photo', 'dolly_photo'])
def test_reference_frames_at_size_byte_for_byte_and_where_the_jacobi_schedule_moves_them(oracle, monkeypatch, tag):
    """process_kenburns of the REFERENCE at 256 x 320 (kernel text executed serially; tests/golden/make_golden.py
    gen_kenburns_at_size) against this package's host logic + its own Inpaint module + the oracle:
      * serial degrid schedule: every frame byte for byte;
      * Jacobi schedule (the product's: DESIGN.md section 2, deviation 1) on the SAME cloud: what it costs against those frames
        on this scene, whose colours are white noise (any pixel that takes another source point moves by up to 255), and
        WHERE -- only pixels whose degridded z differs between the schedules, and filled holes (a fill depends on validity
        along its rays); nowhere else."""
    from ken_burns_effect_amd import common as C, synthetic
    from ken_burns_effect_amd.pointcloud_inpainting import Inpaint
    z = load_golden('kenburns_at_size_' + tag)
    H, W = int(z['H']), int(z['W'])
    torch.set_num_threads(1)
    monkeypatch.setattr(C, '_kernel_set', oracle.OracleKernels(schedule='serial'))
    settings, oc = at_size_scene(z, 'cpu', oracle.depth_to_points)
    net = synthetic.seeded_fill_(Inpaint(), 3).eval()
    with torch.no_grad():
        frames = C.process_kenburns(settings, oc, net)
    assert oc['tensorInpaPoints'].shape[-1] == int(z['n_points'])
    for i, (f, ref) in enumerate(zip(frames, z['frames'])):
        assert np.array_equal(f, ref), 'frame %d under the serial schedule' % i
    ks, kj = oracle.OracleKernels('serial'), oracle.OracleKernels('jacobi')
    st = ks.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], W, H)
    for i, ((focal, sh), ref) in enumerate(zip(C.frame_cameras(settings, oc), z['frames'])):
        fs, _, es = ks.render_frame(st, sh, focal, 120, want_float=True)
        fj, _, ej = kj.render_frame(st, sh, focal, 120, want_float=True)
        zp, _ = oracle.zsplat(oracle.shift_points(st['points'], torch.tensor(sh, dtype=torch.float32)), W, H, focal, 120)
        dz = oracle.degrid(zp, 'serial')[0, 0].numpy().view(np.int32) != oracle.degrid(zp, 'jacobi')[0, 0].numpy().view(np.int32)
        holes = (es[0, 0].numpy() <= 0) | (ej[0, 0].numpy() <= 0)
        moved = np.abs(fs.numpy().astype(np.int32) - fj.numpy().astype(np.int32)).max(axis=2) > 0
        assert np.array_equal(fs.numpy(), ref)
        assert not (moved & ~dz & ~holes).any(), 'frame %d: a pixel moved that is neither a hole nor a pixel whose z the schedules degrid differently' % i
        # measured: KBE 32.3-36.7 dB with 394-509 of 81 920 pixels moved; dolly 33.9-43.5 dB, 84-175 pixels
        assert psnr_u8(fj.numpy(), ref) > JACOBI_FLOOR_DB[tag] and moved.mean() < 0.01, 'frame %d: %.2f dB, %d pixels' % (i, psnr_u8(fj.numpy(), ref), int(moved.sum()))


def test_crop_is_applied_by_default(common):
    z = load_golden('kenburns_dolly')
    settings, oc = _scene(z)
    settings.pop('boolCrop')
    frames = common.process_kenburns(settings, oc, None)
    from oracle import kbe_oracle
    cw, ch = common.crop_size(settings)
    for f, g in zip(frames, z['frames']):
        assert np.array_equal(f, kbe_oracle.crop_resize_u8(g, cw, ch))


def test_process_load_with_disparity_bypass(common):
    from ken_burns_effect_amd import synthetic
    image, disp = synthetic.make_rgbd(40, 48, 9)
    img8 = (image[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    oc = {}
    common.process_load(img8, {'tensorDisparity': disp, 'device': 'cpu'}, oc)
    for k in ('dblFocal', 'dblBaseline', 'intWidth', 'intHeight', 'dblDispmin', 'dblDispmax', 'objectDepthrange', 'tensorRawImage',
              'tensorRawDisparity', 'tensorRawDepth', 'tensorRawPoints', 'tensorRawUnaltered', 'tensorInpaImage',
              'tensorInpaDisparity', 'tensorInpaDepth', 'tensorInpaPoints'):
        assert k in oc
    assert oc['dblBaseline'] == 40.0 and oc['dblFocal'] == 512.0
    assert oc['tensorRawPoints'].shape == (1, 3, 40 * 48)
    assert abs(oc['dblDispmax'] - 40.0) < 1e-4


def test_product_refuses_to_run_without_gpu_library_or_tensors():
    """No silent fallback: CPU tensors are rejected by the HIP binding."""
    from ken_burns_effect_amd import _native
    with pytest.raises(_native.KbeError):
        _native._ptr(torch.zeros(4))


def test_degrid_fast_path_mean_is_the_correctly_rounded_division(tmp_path):
    """kbe_device.h degrid_pixel_fast replaces sum / count by a multiply + one Markstein correction; the C
    program checks it against the division for every float in the band the fast path is used in."""
    import os
    import subprocess
    exe = str(tmp_path / 'markstein_check')
    src = os.path.join(os.path.dirname(__file__), 'markstein_check.c')
    subprocess.check_call(['gcc', '-O2', '-mfma', '-ffp-contract=off', src, '-o', exe, '-lm'])
    out = subprocess.run([exe, '1048576', '8400000'], capture_output=True, text=True)      # 2^20 .. 8 * 1e6 (+ margin)
    n, bad = (int(v) for v in out.stdout.split())
    assert out.returncode == 0 and bad == 0 and n > 4 * 12_000_000


def test_get_masks_plumbing_with_the_oracle_kernel_set(oracle):
    """utils.get_masks (utils/utils.py:248-300): both return forms, per-sample zoom settings, on the CPU oracle."""
    import torch
    from ken_burns_effect_amd import common, synthetic, utils
    common._kernel_set = oracle.OracleKernels('jacobi')
    try:
        H, W, B = 48, 64, 2
        imgs, disps = zip(*[synthetic.make_rgbd(H, W, 7 + b) for b in range(B)])
        image, disp = torch.cat(imgs), torch.cat(disps)
        depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
        zoom = {'objectFrom': {'dblCenterU': [W / 2.0] * B, 'dblCenterV': [H / 2.0] * B, 'intCropWidth': [W] * B, 'intCropHeight': [H] * B},
                'objectTo': {'dblCenterU': [W / 2.0 + 3, W / 2.0 - 2], 'dblCenterV': [H / 2.0, H / 2.0 + 1],
                             'intCropWidth': [int(W * 0.8)] * B, 'intCropHeight': [int(H * 0.8)] * B}}
        camera = {'focal': synthetic.FOCAL, 'baseline': synthetic.BASELINE}
        masks, shift, objs = utils.get_masks(image, disp, depth, zoom, camera)
        assert masks.shape == (B, 1, H, W) and shift.shape == (B, 3, 1) and len(objs) == B
        assert set(torch.unique(masks).tolist()) <= {0.0, 1.0} and 0.0 < float(masks.mean()) < 1.0
        assert not torch.equal(shift[0], shift[1])                      # per-sample zoom settings were used
        render, holes, pts, shift2, _ = utils.get_masks(image, disp, depth, zoom, camera, AFromB=False)
        assert render.shape == (B, 4, H, W) and holes.shape == (B, 1, H, W) and pts.shape == (B, 3, H * W)
        assert torch.equal(shift, shift2)
    finally:
        common._kernel_set = None


def test_shared_reciprocal_division_is_the_correctly_rounded_division(tmp_path):
    """kbe_tiles.h tile_epilogue (resolve): four numerators over one denominator = one IEEE reciprocal + a Markstein step each."""
    import os
    import subprocess
    exe = str(tmp_path / 'markstein_div_check')
    src = os.path.join(os.path.dirname(__file__), 'markstein_div_check.c')
    subprocess.check_call(['gcc', '-O2', '-mfma', '-ffp-contract=off', src, '-o', exe, '-lm'])
    out = subprocess.run([exe, '60000000'], capture_output=True, text=True)
    n, bad = (int(v) for v in out.stdout.split()[-2:])
    assert out.returncode == 0 and bad == 0 and n == 60000000


def test_fp32_image_position_and_cull_equal_the_fp64_forms(tmp_path):
    """kbe_device.h project_xy: `(float) (((double) ix + W/2) - 0.5)` as ONE fp32 addition and `(double) z >= 0.001`
    as an fp32 comparison.  The C program compares bit patterns; here every 1021st fp32 value for 17 sizes (the
    full sweep, stride 1: 7.7e10 comparisons, no mismatch, 2 min 15 s on one core)."""
    import os
    import subprocess
    exe = str(tmp_path / 'centre_offset_check')
    src = os.path.join(os.path.dirname(__file__), 'centre_offset_check.c')
    subprocess.check_call(['gcc', '-O2', '-ffp-contract=off', src, '-o', exe, '-lm'])
    out = subprocess.run([exe, '1021'], capture_output=True, text=True)
    n, bad = (int(v) for v in out.stdout.split()[-2:])
    assert out.returncode == 0 and bad == 0 and n > 70_000_000


def test_host_lanes_two_where_the_link_binds_all_where_the_rendering_does(monkeypatch):
    """_native.host_lanes: the lanes of the frame loop when frames go to pinned host memory (measured table in its docstring)."""
    from ken_burns_effect_amd import _native
    monkeypatch.delenv('KBE_HOST_LANES', raising=False)
    cases = {'bench default (inpainted, 1024^2)': (1137109, 1024, 2), '512^2 inpainted (launch-bound)': (284000, 512, 4),
             'dolly / raw cloud (holes)': (1048576, 1024, 4), 'configs[4]: 16.8 M points': (16777216, 2048, 4),
             '2048^2 inpainted': (4550000, 2048, 2)}
    for name, (n, size, want) in cases.items():
        assert _native.host_lanes(4, n, size, size, 3 * size * size) == want, name
    assert _native.host_lanes(1, 1137109, 1024, 1024, 3 << 20) == 1
    monkeypatch.setenv('KBE_HOST_LANES', '3')
    assert _native.host_lanes(4, 1137109, 1024, 1024, 3 << 20) == 3


def test_lanes_for_delivery_follow_the_measured_render_time():
    """_native.lanes_for_delivery (what HipKernels.delivery_lanes applies to the render time it measures once per cloud): two
    lanes where the link needs 1.5 x longer per frame than the rendering, every lane where the rendering binds."""
    from ken_burns_effect_amd import _native
    fb = 3 * 1024 * 1024                                            # 59 us on the link
    assert _native.lanes_for_delivery(4, 25.0, fb) == 2             # the bench workload: the link binds
    assert _native.lanes_for_delivery(4, 39.0, fb) == 2 and _native.lanes_for_delivery(4, 40.0, fb) == 4
    assert _native.lanes_for_delivery(4, 98.0, fb) == 4             # a dolly zoom: the fill binds
    assert _native.lanes_for_delivery(4, 12.0, 3 * 512 * 512) == 4 and _native.lanes_for_delivery(4, 9.0, 3 * 512 * 512) == 2     # 512^2: 14.8 us on the link
    assert _native.lanes_for_delivery(1, 25.0, fb) == 1 and _native.lanes_for_delivery(8, 5.0, fb) == 2


def test_transfer_groups_follow_the_lanes():
    """_native.transfer_group: up to 32 frames per transfer where the link binds (two lanes), one scatter launch's frames where the
    rendering does (all lanes)."""
    from ken_burns_effect_amd import _native
    assert _native.transfer_group(1024, 2, 12) == -32 and _native.transfer_group(75, 2, 12) == -18 and _native.transfer_group(100, 2, 12) == -25
    assert _native.transfer_group(20, 2, 12) == -16 and _native.transfer_group(3, 2, 12) == -16 and _native.transfer_group(0, 2, 12) == -16      # (render_video caps at the video's length)
    assert _native.transfer_group(256, 4, 8) == -8 and _native.transfer_group(64, 4, 2) == -2 and _native.transfer_group(5, 3, 12) == -12
    assert _native.transfer_group(20, 2, 12, fast_ramp=True) == -16 and _native.transfer_group(50, 2, 12, fast_ramp=True) == -25
    assert _native.transfer_group(100, 1, 12) == -32


def test_video_launch_shape_by_frame_size_and_camera(monkeypatch):
    """_native.video_launch_shape: the table-driven fill for clouds without appended points seen by a camera that zooms out;
    frames per launch by what binds the video; the scatter route is the cloud's (until round 5 a zoom-out took the bucket route)."""
    from ken_burns_effect_amd import _native
    for k in ('KBE_FILL_DIST', 'KBE_FILL_GROUP', 'KBE_FUSED'):
        monkeypatch.delenv(k, raising=False)
    cls = [c for c in vars(_native).values() if isinstance(c, type) and hasattr(c, 'video_launch_shape')][0]
    shape = lambda state, cams, batch=None, **kw: cls.video_launch_shape(None, state, cams, batch, **kw)       # noqa: E731
    still = [(512.0, (0.0, 0.0, 0.0))] * 8
    zoom = [(512.0 - 40.0 * i, (0.0, 0.0, -20.0 * i)) for i in range(8)]
    inpainted = {'W': 1024, 'H': 1024, 'N': 1137109, 'cloud_focal': 512.0, 'fused': True}
    raw = {'W': 1024, 'H': 1024, 'N': 1048576, 'cloud_focal': 512.0, 'fused': True}
    # the fused route: four frames per launch left in HBM, twelve where the link binds (KBE_VIDEO_GROUP: bits 5-8); a zoom-out of a
    # cloud without appended points fills with the tables, eight frames per scatter launch
    assert shape(inpainted, still) == (3 << 1, 4, True) and shape(inpainted, still, to_host=True) == (11 << 5, 12, True)
    assert shape(inpainted, zoom) == (3 << 1, 4, True)
    assert shape(raw, still) == (3 << 1, 4, True)
    assert shape(raw, zoom) == (1 | (7 << 5), 8, True)
    assert shape(raw, zoom, batch=8) == (1, 1, True), 'the staged ring renders one frame per launch'
    assert shape({'W': 512, 'H': 512, 'N': 300000, 'cloud_focal': 512.0, 'fused': True}, still) == (3 << 1, 4, True)
    # a cloud denser than the raster on the fused route (configs[4]: 16.8 M points at 2048^2): three frames per launch, delivered or left in
    # HBM (two until round 6, from the blit hand-off's days: profiles/r06_config4_groups.txt)
    config4 = {'W': 2048, 'H': 2048, 'N': 4 * 2048 * 2048, 'cloud_focal': 1024.0, 'fused': True}
    assert shape(config4, still, to_host=True) == (2 << 1, 3, True) and shape(config4, still) == (2 << 1, 3, True)
    # the bucket route (a cloud denser than the raster: prepare_cloud leaves `fused` off)
    dense = lambda size, n: {'W': size, 'H': size, 'N': n, 'cloud_focal': 512.0, 'fused': False}    # noqa: E731
    assert shape(dense(1024, 4 << 20), still) == (0, 1, False)
    assert shape(dense(512, 1 << 20), still) == (3 << 1, 4, False)
    assert shape(dense(768, 2 << 20), still) == (1 << 1, 2, False)
    monkeypatch.setenv('KBE_FILL_GROUP', '3')
    assert shape(inpainted, still) == (2 << 1, 3, True)
    monkeypatch.setenv('KBE_FILL_DIST', '0')
    assert shape(raw, zoom) == (2 << 1, 3, True)
    assert shape(dict(raw, fused=False), zoom) == (2 << 1, 3, False), 'the route is the state\'s (prepare_cloud: KBE_FUSED=0 / 1 force it there)'


def test_degrid_schedule_switch_selects_the_serial_route(monkeypatch):
    """KBE_DEGRID (round 6): jacobi -- the fused tile launch, the default -- or serial: the same HIP library behind the stage-by-stage
    kernel set that reproduces a serial execution of the reference (no render_video: the frame loop goes frame by frame).  Read per call."""
    from ken_burns_effect_amd import _native
    monkeypatch.delenv('KBE_DEGRID', raising=False)
    default = _native.kernels()
    assert isinstance(default, _native.HipKernels) and _native.degrid_schedule() == 'jacobi'
    monkeypatch.setenv('KBE_DEGRID', 'serial')
    serial = _native.kernels()
    assert isinstance(serial, _native.HipSerialScheduleKernels) and serial.K is default and serial.name == 'hip-serial'
    assert not hasattr(serial, 'render_video') and serial.lib is default.lib                      # everything else is the library's
    assert _native.kernels() is serial                                                             # one per process
    monkeypatch.setenv('KBE_DEGRID', 'gauss-seidel')
    with pytest.raises(_native.KbeError):
        _native.kernels()
    monkeypatch.delenv('KBE_DEGRID')
    assert _native.kernels() is default


# What HipKernels.render_video passed to kbe_render_video before video_shape.call_shape existed: (case, cloud, frames, zooms out,
# to host, batch argument, lanes chosen, switches away from their defaults, budget in sets or None) -> (batch, frames per launch,
# flags, scratch sets).  RECORDED rows are the arguments of real calls, taken with a shim in front of the library entry on an
# MI355X at the commit before the split (clouds of bench.build_scene); the rows marked COMPOSED could not be reached that way and
# were put together by hand from that commit's own video_launch_shape, transfer_group and host_lanes, run on the CPU.
_INPAINTED, _RAW, _DENSE = (1137109, 1024, 1024, True), (1048576, 1024, 1024, True), (4194304, 1024, 1024, True)
_BUCKET512, _BUCKET768, _BUCKET1024 = (280049, 512, 512, False), (617619, 768, 768, False), (1137109, 1024, 1024, False)
_BUDGET_SHAPE = (288 * 224, 288, 224, True)          # test_hip_parity.py::test_scratch_budget_falls_back_...: a raw 288 x 224 cloud, KBE_FUSED=1
_SET = 1.0                                           # (any budget in MB: call_shape only asks whether the switch is set)
_CALL_SHAPE_ROWS = [
    # the bench default: inpainted 1024^2, delivered
    ('bench default, 20 frames', _INPAINTED, 20, False, True, None, 2, {}, None, (-16, 12, 8544, 24)),
    ('bench default, 75 frames', _INPAINTED, 75, False, True, None, 2, {}, None, (-18, 12, 8544, 24)),
    ('bench default, 256 frames, two lanes', _INPAINTED, 256, False, True, None, 2, {}, None, (-32, 12, 8544, 24)),
    ('bench default, 1024 frames (COMPOSED)', _INPAINTED, 1024, False, True, None, 2, {}, None, (-32, 12, 8544, 24)),
    ('bench default, 1 frame', _INPAINTED, 1, False, True, None, 2, {}, None, (-1, 12, 8544, 24)),
    ('bench default, 3 frames', _INPAINTED, 3, False, True, None, 2, {}, None, (-3, 12, 8544, 24)),
    ('256 frames on three lanes', _INPAINTED, 256, False, True, None, 3, {}, None, (-12, 12, 8544, 36)),
    ('256 frames on four lanes', _INPAINTED, 256, False, True, None, 4, {}, None, (-12, 12, 8544, 48)),
    # left in HBM
    ('left in HBM, 20 frames', _INPAINTED, 20, False, False, None, 4, {}, None, (0, 4, 6, 16)),
    ('left in HBM, 1 frame', _INPAINTED, 1, False, False, None, 4, {}, None, (0, 4, 6, 16)),
    ('left in HBM, batch=-8 is ignored', _INPAINTED, 20, False, False, -8, 4, {}, None, (0, 4, 6, 16)),
    ('left in HBM, batch=8 is ignored', _INPAINTED, 20, False, False, 8, 4, {}, None, (0, 4, 6, 16)),
    # a dolly zoom-out of a raw cloud
    ('dolly, 20 frames to host on four lanes', _RAW, 20, True, True, None, 4, {}, None, (-8, 8, 8425, 32)),
    ('dolly, 3 frames to host', _RAW, 3, True, True, None, 4, {}, None, (-3, 8, 8425, 32)),
    ('dolly, 256 frames to host on two lanes', _RAW, 256, True, True, None, 2, {}, None, (-32, 8, 8425, 16)),
    ('dolly, left in HBM', _RAW, 75, True, False, None, 4, {}, None, (0, 8, 225, 32)),
    # a cloud denser than the raster
    ('dense, 20 frames to host', _DENSE, 20, False, True, None, 4, {}, None, (-3, 3, 8196, 12)),
    ('dense, left in HBM', _DENSE, 20, False, False, None, 4, {}, None, (0, 3, 4, 12)),
    # the bucket route at three frame sizes
    ('bucket 512^2 to host', _BUCKET512, 20, False, True, None, 4, {}, None, (-4, 4, 8198, 16)),
    ('bucket 512^2 in HBM', _BUCKET512, 20, False, False, None, 4, {}, None, (0, 4, 6, 16)),
    ('bucket 768^2 to host', _BUCKET768, 20, False, True, None, 2, {}, None, (-16, 2, 8194, 4)),
    ('bucket 768^2 in HBM', _BUCKET768, 20, False, False, None, 4, {}, None, (0, 2, 2, 8)),
    ('bucket 1024^2 to host', _BUCKET1024, 20, False, True, None, 2, {}, None, (-16, 1, 8192, 2)),
    ('bucket 1024^2 in HBM', _BUCKET1024, 20, False, False, None, 4, {}, None, (0, 1, 0, 4)),
    # an explicit batch
    ('batch=0: per-frame delivery', _INPAINTED, 20, False, True, 0, 2, {}, None, (0, 12, 352, 24)),
    ('batch=-8', _INPAINTED, 20, False, True, -8, 2, {}, None, (-8, 12, 8544, 24)),
    ('batch=8: the staged ring', _INPAINTED, 20, False, True, 8, 2, {}, None, (8, 1, 0, 2)),
    ('batch=8 on the bucket route', _BUCKET512, 20, False, True, 8, 4, {}, None, (8, 1, 0, 4)),
    ('batch=0 on the bucket route', _BUCKET512, 20, False, True, 0, 4, {}, None, (0, 4, 6, 16)),
    # each switch away from its default, one at a time
    ('KBE_FILL_DIST=1 to host', _INPAINTED, 20, False, True, None, 2, {'fill_dist': True}, None, (-16, 8, 8425, 16)),
    ('KBE_FILL_DIST=1 in HBM', _INPAINTED, 20, False, False, None, 4, {'fill_dist': True}, None, (0, 8, 225, 32)),
    ('KBE_FILL_DIST=0, dolly', _RAW, 75, True, True, None, 4, {'fill_dist': False}, None, (-12, 12, 8544, 48)),
    ('KBE_FILL_GROUP=3 to host', _INPAINTED, 20, False, True, None, 2, {'fill_group': 3}, None, (-16, 3, 8196, 6)),
    ('KBE_FILL_GROUP=7 in HBM', _INPAINTED, 20, False, False, None, 4, {'fill_group': 7}, None, (0, 7, 192, 28)),
    ('KBE_FILL_GROUP=40 in HBM', _INPAINTED, 20, False, False, None, 4, {'fill_group': 40}, None, (0, 12, 352, 48)),
    ('KBE_FILL_GROUP=7, dolly', _RAW, 75, True, True, None, 4, {'fill_group': 7}, None, (-7, 7, 8393, 28)),
    ('KBE_HOST_LANES=1', _INPAINTED, 20, False, True, None, 1, {'host_lanes': 1}, None, (-16, 12, 8544, 12)),
    ('KBE_HOST_LANES=3', _INPAINTED, 20, False, True, None, 3, {'host_lanes': 3}, None, (-12, 12, 8544, 36)),
    ('KBE_HOST_LANES=1, dolly', _RAW, 75, True, True, None, 1, {'host_lanes': 1}, None, (-32, 8, 8425, 8)),
    ('KBE_DELIVERY_BATCH=-4', _INPAINTED, 20, False, True, None, 2, {'delivery_batch': -4}, None, (-4, 12, 8544, 24)),
    ('KBE_DELIVERY_BATCH=6', _INPAINTED, 20, False, True, None, 2, {'delivery_batch': 6}, None, (6, 1, 0, 2)),
    ('KBE_DELIVERY_BATCH=6, dolly', _RAW, 75, True, True, None, 4, {'delivery_batch': 6}, None, (6, 1, 9, 4)),
    ('KBE_DELIVERY_BATCH=-4 in HBM', _INPAINTED, 20, False, False, None, 4, {'delivery_batch': -4}, None, (0, 4, 6, 16)),
    ('KBE_RAMP=fast to host', _INPAINTED, 20, False, True, None, 2, {'fast_ramp': True}, None, (-16, 12, 9568, 24)),
    ('KBE_RAMP=fast in HBM', _INPAINTED, 20, False, False, None, 4, {'fast_ramp': True}, None, (0, 4, 1030, 16)),
    ('KBE_FREE_TRANSFERS=1 to host', _INPAINTED, 20, False, True, None, 2, {'free_transfers': True}, None, (-16, 12, 8552, 24)),
    ('KBE_FREE_TRANSFERS=1 in HBM', _INPAINTED, 20, False, False, None, 4, {'free_transfers': True}, None, (0, 4, 6, 16)),
    ('KBE_FREE_TRANSFERS=0, dolly', _RAW, 75, True, True, None, 4, {'free_transfers': False}, None, (-8, 8, 8417, 32)),
    ('KBE_EVEN_GROUPS=1 to host', _INPAINTED, 20, False, True, None, 2, {'even_groups': True}, None, (-16, 12, 8560, 24)),
    ('KBE_EVEN_GROUPS=1 in HBM', _INPAINTED, 20, False, False, None, 4, {'even_groups': True}, None, (0, 4, 22, 16)),
    ('KBE_AHEAD=0 to host', _INPAINTED, 20, False, True, None, 2, {'no_ahead': True}, None, (-16, 12, 9056, 24)),
    ('KBE_AHEAD=0 in HBM', _INPAINTED, 20, False, False, None, 4, {'no_ahead': True}, None, (0, 4, 518, 16)),
    ('KBE_FUSED_CAP=lean to host', _INPAINTED, 20, False, True, None, 2, {'build_bits': 2048}, None, (-16, 12, 10592, 24)),
    ('KBE_FUSED_CAP=roomy in HBM', _INPAINTED, 20, False, False, None, 4, {'build_bits': 4096}, None, (0, 4, 4102, 16)),
    ('KBE_HANDOFF=blit', _INPAINTED, 20, False, True, None, 2, {'sdma': False}, None, (-16, 12, 352, 24)),
    ('KBE_HANDOFF=blit, dolly', _RAW, 75, True, True, None, 4, {'sdma': False}, None, (-8, 8, 233, 32)),
    ('KBE_INJECT_HANDOFF_FAULT=1 (COMPOSED)', _INPAINTED, 20, False, True, None, 2, {'inject_fault': True}, None, (-16, 12, 8544 | 32768, 24)),
    ('KBE_INJECT_HANDOFF_TIMEOUT=1 (COMPOSED)', _INPAINTED, 20, False, True, None, 2, {'inject_timeout': True}, None, (-16, 12, 8544 | 65536, 24)),
    ('the hooks need the SDMA hand-off (COMPOSED)', _INPAINTED, 20, False, True, None, 2, {'inject_fault': True, 'inject_timeout': True, 'sdma': False}, None, (-16, 12, 352, 24)),
    ('the hooks, per-frame delivery (COMPOSED)', _INPAINTED, 20, False, True, 0, 2, {'inject_fault': True, 'inject_timeout': True}, None, (0, 12, 352, 24)),
    ('the hooks, left in HBM (COMPOSED)', _INPAINTED, 20, False, False, None, 4, {'inject_fault': True, 'inject_timeout': True}, None, (0, 4, 6, 16)),
    # KBE_SCRATCH_BUDGET_MB; the transfer group (batch) stays that of the uncut shape
    ('budget 9 sets, two lanes', _INPAINTED, 20, False, True, None, 2, {'scratch_budget_mb': _SET}, 9, (-16, 3, 8196, 6)),
    ('budget 9 sets, in HBM', _INPAINTED, 20, False, False, None, 4, {'scratch_budget_mb': _SET}, 9, (0, 2, 2, 8)),
    ('budget 9 sets, four lanes to host', _INPAINTED, 20, False, True, None, 4, {'scratch_budget_mb': _SET}, 9, (-12, 1, 8192, 4)),
    ('budget < 1 set, two lanes', _INPAINTED, 20, False, True, None, 2, {'scratch_budget_mb': _SET}, 4, (-16, 1, 8192, 2)),
    ('budget < 1 set, in HBM', _INPAINTED, 20, False, False, None, 4, {'scratch_budget_mb': _SET}, 4, (0, 1, 0, 4)),
    ('budget 21 sets, two lanes', _INPAINTED, 20, False, True, None, 2, {'scratch_budget_mb': _SET}, 21, (-16, 6, 8352, 12)),
    ('budget 21 sets, in HBM: not binding', _INPAINTED, 20, False, False, None, 4, {'scratch_budget_mb': _SET}, 21, (0, 4, 6, 16)),
    ('budget 21 sets, four lanes to host', _INPAINTED, 20, False, True, None, 4, {'scratch_budget_mb': _SET}, 21, (-12, 3, 8196, 12)),
    ('budget 9 sets, dolly', _RAW, 75, True, True, None, 4, {'scratch_budget_mb': _SET}, 9, (-8, 2, 8203, 8)),
    ('budget < 1 set, dolly', _RAW, 75, True, True, None, 4, {'scratch_budget_mb': _SET}, 4, (-8, 1, 8201, 4)),
    ('budget 21 sets, dolly', _RAW, 75, True, True, None, 4, {'scratch_budget_mb': _SET}, 21, (-8, 4, 8207, 16)),
    # the shape of the GPU test of the budget, whose assertions are 8 and 4 sets (COMPOSED)
    ('GPU budget test, no budget (COMPOSED)', _BUDGET_SHAPE, 40, True, False, None, 4, {}, None, (0, 8, 225, 32)),
    ('GPU budget test, nine sets (COMPOSED)', _BUDGET_SHAPE, 40, True, False, None, 4, {'scratch_budget_mb': _SET}, 9, (0, 2, 3, 8)),
    ('GPU budget test, less than one set (COMPOSED)', _BUDGET_SHAPE, 40, True, False, None, 4, {'scratch_budget_mb': _SET}, 4, (0, 1, 1, 4)),
]


@pytest.mark.parametrize('row', _CALL_SHAPE_ROWS, ids=[r[0] for r in _CALL_SHAPE_ROWS])
def test_call_shape_passes_what_render_video_passed(row):
    """video_shape.call_shape on plain values: all six fields of the call's shape against the table above."""
    from ken_burns_effect_amd import video_shape
    _, (N, W, H, fused), n, zooms_out, to_host, batch, lanes, switches, budget, (want_batch, want_group, want_flags, want_sets) = row
    sw = video_shape.DEFAULTS._replace(**switches)
    budget_sets = (lambda: 1 << 20) if budget is None else (lambda: budget)        # (no switch: half of a device's free memory, never binding here)
    got = video_shape.call_shape(N, W, H, fused, n, zooms_out, to_host, batch, lanes, sw, 0, budget_sets)
    assert got == video_shape.CallShape(lanes=lanes, batch=want_batch, group=want_group, flags=want_flags, fused=fused, sets=want_sets)
    assert got.sets == got.group * got.lanes


def test_call_shape_asks_for_the_budget_only_when_it_has_to():
    """The budget reads the device's free memory (~10 us of a call): not asked while the sets the cloud holds do and
    KBE_SCRATCH_BUDGET_MB is unset, nor when one frame per launch renders on the lanes' own sets."""
    from ken_burns_effect_amd import video_shape
    asked = []

    def budget():
        asked.append(1)
        return 1 << 20
    shape = lambda cloud, to_host, lanes, held, sw=video_shape.DEFAULTS, batch=None: video_shape.call_shape(      # noqa: E731
        *cloud, 20, False, to_host, batch, lanes, sw, held, budget)
    assert shape(_INPAINTED, True, 2, 24).sets == 24 and shape(_INPAINTED, False, 4, 48).sets == 16 and not asked
    assert shape(_BUCKET1024, False, 4, 0).sets == 4 and shape(_INPAINTED, True, 2, 0, batch=8).sets == 2 and not asked
    assert shape(_INPAINTED, True, 2, 23).sets == 24 and len(asked) == 1
    assert shape(_INPAINTED, True, 2, 0).sets == 24 and len(asked) == 2
    assert shape(_INPAINTED, True, 2, 24, video_shape.DEFAULTS._replace(scratch_budget_mb=1e6)).sets == 24 and len(asked) == 3


def test_video_switches_reads_the_environment_once_into_a_record(monkeypatch):
    """_native.video_switches: every switch of a video call, parsed; unset = video_shape.DEFAULTS; read per call."""
    from ken_burns_effect_amd import _native, video_shape
    names = ('KBE_FILL_DIST', 'KBE_FILL_GROUP', 'KBE_HOST_LANES', 'KBE_DELIVERY_BATCH', 'KBE_RAMP', 'KBE_FREE_TRANSFERS', 'KBE_EVEN_GROUPS', 'KBE_AHEAD',
             'KBE_FUSED_CAP', 'KBE_HANDOFF', 'KBE_INJECT_HANDOFF_FAULT', 'KBE_INJECT_HANDOFF_TIMEOUT', 'KBE_SCRATCH_BUDGET_MB')
    for k in names:
        monkeypatch.delenv(k, raising=False)
    assert _native.video_switches() == video_shape.DEFAULTS
    cases = [('KBE_FILL_DIST', '1', {'fill_dist': True}), ('KBE_FILL_DIST', '0', {'fill_dist': False}), ('KBE_FILL_DIST', 'auto', {}),
             ('KBE_FILL_GROUP', '7', {'fill_group': 7}), ('KBE_FILL_GROUP', '', {}), ('KBE_HOST_LANES', '3', {'host_lanes': 3}), ('KBE_HOST_LANES', '0', {'host_lanes': 0}),
             ('KBE_DELIVERY_BATCH', '-4', {'delivery_batch': -4}), ('KBE_RAMP', 'fast', {'fast_ramp': True}), ('KBE_RAMP', 'classic', {}),
             ('KBE_FREE_TRANSFERS', '1', {'free_transfers': True}), ('KBE_FREE_TRANSFERS', '0', {'free_transfers': False}), ('KBE_EVEN_GROUPS', '1', {'even_groups': True}),
             ('KBE_AHEAD', '0', {'no_ahead': True}), ('KBE_AHEAD', '1', {}), ('KBE_FUSED_CAP', 'lean', {'build_bits': _native.KBE_VIDEO_FUSED_LEAN}),
             ('KBE_FUSED_CAP', 'roomy', {'build_bits': _native.KBE_VIDEO_FUSED_ROOMY}), ('KBE_HANDOFF', 'blit', {'sdma': False}), ('KBE_HANDOFF', 'sdma', {}),
             ('KBE_INJECT_HANDOFF_FAULT', '1', {'inject_fault': True}), ('KBE_INJECT_HANDOFF_TIMEOUT', '1', {'inject_timeout': True}),
             ('KBE_SCRATCH_BUDGET_MB', '1', {'scratch_budget_mb': 1.0}), ('KBE_SCRATCH_BUDGET_MB', '0', {'scratch_budget_mb': 0.0})]
    for name, value, fields in cases:
        monkeypatch.setenv(name, value)
        assert _native.video_switches() == video_shape.DEFAULTS._replace(**fields), (name, value)
        monkeypatch.delenv(name)
    assert set(names) == {c[0] for c in cases}
    monkeypatch.setenv('KBE_FUSED_CAP', 'lean')
    assert _native.fused_build_bits() == _native.KBE_STAGE_FUSED_LEAN and _native.fused_build_bits(video=True) == _native.KBE_VIDEO_FUSED_LEAN
    monkeypatch.delenv('KBE_FUSED_CAP')
    monkeypatch.setenv('KBE_DELIVERY_BATCH', 'many')
    with pytest.raises(_native.KbeError, match="KBE_DELIVERY_BATCH='many' is not an integer"):
        _native.video_switches()


def test_the_shape_of_a_call_is_decided_without_gpu_library_or_environment():
    """video_shape is plain Python on plain values: no torch, no ctypes, no os."""
    import ast
    from ken_burns_effect_amd import video_shape
    tree = ast.parse(open(video_shape.__file__).read())
    imported = {a.name.split('.')[0] for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names}
    imported |= {(node.module or '').split('.')[0] for node in ast.walk(tree) if isinstance(node, ast.ImportFrom)}
    assert imported == {'collections'}
