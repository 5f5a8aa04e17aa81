"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the golden vectors.

Bars (BASELINE.json north_star): z-buffer and winner indices bit-exact; byte / index / mask work
bit-exact; accumulated colour within fp32 summation-order noise (tolerances written at each
assertion); frames within 1e-3 dB PSNR of the oracle's.
"""
import os

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, load_golden

pytestmark = pytest.mark.gpu

RENDER_CASES = ['render_f512', 'render_f409', 'render_f153', 'render_noise', 'render_b2c7']


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()          # raises if libkbe_hip.so is missing: no fallback


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def c(t):
    return t.detach().cpu().numpy()


def _baseline(z):
    b = float(z['baseline'])
    return int(b) if bool(z['baseline_is_int']) else b


def psnr(a, b, peak):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 200.0 if mse == 0 else 10.0 * np.log10(peak * peak / mse)


# ---------------------------------------------------------------------------------------
# render_pointcloud stages on the golden inputs
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', RENDER_CASES)
def test_zbuffer_and_winners_bit_exact(K, oracle, case):
    z = load_golden(case)
    W, H, F, Bl = int(z['W']), int(z['H']), float(z['focal']), _baseline(z)
    zkeys, winner = K.zsplat(g(z['points']), W, H, F, Bl, want_winner=True)
    assert_bits_equal(c(K.zkeys_decode(zkeys)), z['zee_pre_fma'], 'pre-degrid z-buffer vs reference')
    _, ow = oracle.zsplat(torch.from_numpy(z['points']), W, H, F, Bl, want_winner=True)
    assert np.array_equal(c(winner), ow.numpy()), 'winner pixel index per point vs oracle'
    if 'winner_fma' in z.files:
        assert np.array_equal(c(winner), z['winner_fma']), 'winner pixel index per point vs reference'


@pytest.mark.parametrize('case', RENDER_CASES)
def test_degrid_jacobi_bit_exact(K, oracle, case):
    z = load_golden(case)
    pre = torch.from_numpy(z['zee_pre_fma'])
    want = oracle.degrid(pre, 'jacobi').numpy()
    assert_bits_equal(c(K.degrid(zee=g(z['zee_pre_fma']))), want, 'degrid from fp32')
    zkeys, _ = K.zsplat(g(z['points']), int(z['W']), int(z['H']), float(z['focal']), _baseline(z))
    assert_bits_equal(c(K.degrid(zkeys=zkeys)), want, 'degrid from keys')


@pytest.mark.parametrize('case', RENDER_CASES)
def test_accumulate_and_normalize(K, oracle, case):
    z = load_golden(case)
    F, Bl = float(z['focal']), _baseline(z)
    # same z-buffer as the reference run (serial schedule) so that acc is comparable to the golden
    acc = c(K.accumulate(g(z['points']), g(z['data']), g(z['zee_serial_fma']), F, Bl))
    want = z['acc_fma']
    # atomic order differs from point-index order: a few ulp of the largest partial sum per pixel
    tol = 1e-5 * np.maximum(np.abs(want), 1.0)
    assert (np.abs(acc - want) <= tol).all()
    assert np.array_equal(acc == 0, want == 0), 'exactly the same pixels/channels are touched'
    render, existing = K.normalize(g(want))
    assert_bits_equal(c(render), z['render_fma'], 'normalise')
    assert_bits_equal(c(existing), z['existing_fma'], 'existing')


@pytest.mark.parametrize('case', RENDER_CASES)
def test_render_pointcloud_whole(K, oracle, case):
    z = load_golden(case)
    W, H, F, Bl = int(z['W']), int(z['H']), float(z['focal']), _baseline(z)
    render, existing = K.render_pointcloud(g(z['points']), g(z['data']), W, H, F, Bl)
    r0, e0 = oracle.render_pointcloud(torch.from_numpy(z['points']), torch.from_numpy(z['data']), W, H, F, Bl, 'jacobi')
    assert np.array_equal(c(existing) > 0, e0.numpy() > 0), 'hole mask identical'
    assert np.abs(c(existing) - e0.numpy()).max() <= 1e-5 * max(1.0, float(e0.max()))
    scale = np.maximum(np.abs(r0.numpy()), 1.0)
    assert (np.abs(c(render) - r0.numpy()) <= 2e-5 * scale).all()


def _random_focal_baseline_pairs():
    """Eight (F, B) with F * B in 10^[-2, 9] (fixed seed), B a float or an int as the draw has it; most products are not fp32 values."""
    rng = np.random.default_rng(470)
    pairs = []
    for k, exponent in enumerate(rng.permutation(np.linspace(-2.0, 9.0, 8))):
        baseline = int(rng.integers(1, 400)) if k % 2 else float(rng.uniform(0.01, 400.0))
        fb = 10.0 ** (exponent + rng.uniform(-0.4, 0.4))
        pairs.append((float(min(max(fb, 0.01), 1e9) / baseline), baseline))
    assert sum(float(np.float32(f * b)) != f * b for f, b in pairs) >= 4
    return pairs


def _dbl_error_depths(fb, n_random, n_boundary, rng):
    """Depths for the division-free dblError: random ones, tiny / huge ones, the floats around the fp32 rounding boundaries of
    1e6 - fb / z for THIS fb, and the floats around 16.0 (project_err_fast: pz >= 16)."""
    zs = [rng.uniform(16.0, 60000.0, n_random), rng.uniform(0.001, 20.0, n_random // 20), 10.0 ** rng.uniform(-3, 7, n_random // 20)]
    # boundaries: Q = (n + 0.5) / 16  <=>  z = fb / Q - 1e-7; take the floats around each
    n = rng.integers(1, 16 * 4000, n_boundary).astype(np.float64)
    zb = (fb / ((n + 0.5) / 16.0) - 1e-7).astype(np.float32)
    for start in (zb, np.full(1, 16.0, np.float32)):
        for k in range(-3, 4):
            z = start.copy()
            for _ in range(abs(k)):
                z = np.nextafter(z, np.float32(np.inf if k > 0 else -np.inf))
            zs.append(z)
    return np.concatenate([np.asarray(v, dtype=np.float32) for v in zs])


def _fast_dbl_error_is_exact(K, focal, baseline, n_random=4_000_000, n_boundary=300_000):
    fb = focal * baseline
    z = _dbl_error_depths(fb, n_random, n_boundary, np.random.default_rng(11))
    fast, exact = K.selftest_err(torch.from_numpy(z).cuda(), focal, baseline)
    with np.errstate(over='ignore'):
        want = (1000000.0 - fb / (z.astype(np.float64) + 0.0000001)).astype(np.float32)
    assert_bits_equal(c(exact), want, 'fp64 expression on the GPU vs numpy')
    assert_bits_equal(c(fast), want, 'fast path')
    return z


@pytest.mark.parametrize('focal,baseline', [(512.0, 120), (409.6, 120), (153.60000000000002, 40.0), (192.0, 120)])
def test_fast_dbl_error_is_exact(K, focal, baseline):
    """The division-free dblError of the frame loop against the literal fp64 expression (on the GPU and in
    numpy): random depths, tiny / huge depths, and depths placed right on the fp32 rounding boundaries of
    1e6 - F*B/z (where the fast path must notice that it cannot decide and fall back)."""
    _fast_dbl_error_is_exact(K, focal, baseline)


# B as a float and as an int; products over 10^[-2, 9]; F * B >= 7.6e6 * 16 (depths from 16 on leave the fast path through s >= 7.6e6); F * B < 1
WIDER_PAIRS = [(512.0, 120.0), (409.6, 120.0), (153.60000000000002, 40)] + _random_focal_baseline_pairs() + [(4096.0, 30000.0), (0.5, 1.5), (0.5, 1)]


@pytest.mark.parametrize('focal,baseline', WIDER_PAIRS, ids=['%.6g-%r' % (f, round(b, 3)) for f, b in WIDER_PAIRS])
def test_fast_dbl_error_is_exact_at_other_products(K, focal, baseline):
    """The same at (F, B) pairs beyond the synthetic scenes' (test_fast_dbl_error_is_exact's assertions, about a million depths each)."""
    z = _fast_dbl_error_is_exact(K, focal, baseline, n_random=700_000, n_boundary=40_000)
    assert 900_000 < z.size < 1_200_000
    if focal * baseline >= 7600000.0 * 16.0:
        assert (16.0 * np.float32(focal * baseline) / z[z >= 16.0] >= np.float32(7600000.0)).sum() > 1000


def test_fast_dbl_error_is_exact_at_the_focals_of_a_dolly(K):
    """... and at the focals common.frame_cameras hands the frames of a dolly zoom (common._camera_at: a different one per step)."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((256, 256), dolly=True)
    cams = common.frame_cameras(dict(settings, dblSteps=[0.0, 0.25, 0.5, 0.75, 1.0]), oc)
    focals = [focal for focal, _ in cams]
    assert len(set(focals)) == 5
    for focal in focals:
        _fast_dbl_error_is_exact(K, focal, oc['dblBaseline'], n_random=700_000, n_boundary=40_000)


def test_unscaled_division_is_the_ieee_division(K):
    """div_unscaled (kbe_device.h: the reciprocal estimate, its refinement, the quotient and two residual corrections -- what the
    compiler's fp32 division is without v_div_scale / v_div_fixup) against `/` on the GPU and against numpy, on the operands the
    frame loop gives it -- (F - z) / -z of common.py:457-459 for depths from the near plane up, 1 / (w + 1e-7) of :686 -- and on
    random operands over the whole range its callers guarantee (exponents within +-100 of 1, a zero numerator)."""
    rng = np.random.default_rng(5)
    n = 6_000_000
    nums, dens = [], []
    for F in (512.0, 409.6, 153.60000000000002, 1536.0):
        z = np.concatenate([10.0 ** rng.uniform(-3, 6, n // 8), rng.uniform(0.001, 4.0 * F, n // 8),
                            np.nextafter(np.float32(F), np.float32(0), dtype=np.float32) * np.ones(4), np.float32(F) * np.ones(4)]).astype(np.float32)
        z = z[z >= np.float32(0.001)]
        nums.append(np.float32(F) - z)
        dens.append(-z)
    w = np.concatenate([rng.uniform(0, 8, n // 4), 10.0 ** rng.uniform(-12, 7, n // 4), np.zeros(8)]).astype(np.float32)
    nums.append(np.ones_like(w))
    dens.append(w + np.float32(0.0000001))
    e = rng.integers(27, 227, n, dtype=np.uint32)        # biased exponents 27..226: |x| in [2^-100, 2^100)
    m = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    sg = rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    a = (sg | (e << np.uint32(23)) | m).view(np.float32)
    e2 = np.clip(e.astype(np.int64) + rng.integers(-90, 91, n), 27, 226).astype(np.uint32)
    b = ((rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)) | (e2 << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)).view(np.float32)
    a[:1000] = 0.0
    nums.append(a)
    dens.append(b)
    num, den = np.concatenate(nums), np.concatenate(dens)
    fast, ieee = K.selftest_division(torch.from_numpy(num).cuda(), torch.from_numpy(den).cuda())
    with np.errstate(all='ignore'):
        want = (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)      # the double quotient rounds to the fp32 one (no double rounding: 53 >= 2 * 24 + 2)
    assert_bits_equal(c(ieee), want, 'the compiler\'s division vs numpy')
    assert_bits_equal(c(fast), want, 'div_unscaled')


def test_shift_fused_equals_shift_then_render(K):
    z = load_golden('render_f512')
    W, H, F, Bl = int(z['W']), int(z['H']), float(z['focal']), _baseline(z)
    pts = g(z['points'])
    shift = [3.25, -1.5, -12.0]
    a, wa = K.zsplat(K.shift_points(pts, shift), W, H, F, Bl, want_winner=True)
    b, wb = K.zsplat(pts, W, H, F, Bl, shift3=shift, want_winner=True)
    assert torch.equal(a, b) and torch.equal(wa, wb)


# ---------------------------------------------------------------------------------------
# fill, torch glue
# ---------------------------------------------------------------------------------------

def test_fill_bit_exact(K):
    z = load_golden('fill')
    for tag in ('a', 'b', 'allholes'):
        out = K.fill_disocclusion(g(z['input_' + tag]), g(z['depth_' + tag]))
        assert_bits_equal(c(out), z['output_' + tag], 'fill ' + tag)
    out = K.fill_disocclusion(g(z['input_allholes']), g(z['depth_allholes']) + 1.0)
    assert_bits_equal(c(out), z['output_noholes'], 'no holes')


def test_torch_glue_bit_exact(K, oracle):
    z = load_golden('torch_helpers')
    for tag in 'abc':
        out = K.depth_to_points(g(z['d2p_depth_' + tag]), float(z['d2p_focal_' + tag]))
        assert_bits_equal(c(out), z['d2p_points_' + tag], 'depth_to_points')
    for i in range(3):
        out = K.shift_points(g(z['ps_points']), g(z['ps_shift_%d' % i]))
        assert_bits_equal(c(out), z['ps_out_%d' % i], 'process_shift')
    for tag in 'ab':
        x = z['sf_input_' + tag]
        for kind in ('median-3', 'median-5'):
            assert_bits_equal(c(K.spatial_filter(g(x), kind)), z['sf_%s_%s' % (kind, tag)], kind)
        lap = c(K.spatial_filter(g(x), 'laplacian'))
        assert_bits_equal(lap, oracle.spatial_filter(torch.from_numpy(x), 'laplacian').numpy(), 'laplacian vs oracle')
        assert np.abs(lap - z['sf_laplacian_' + tag]).max() <= 16 * np.finfo(np.float32).eps * np.abs(x).max()
    assert_bits_equal(c(K.spatial_filter(g(z['sf_input_mask']), 'median-5')), z['sf_median-5_mask'], 'median-5 mask')
    assert K.spatial_filter(g(z['sf_input_mask']), 'gaussian') is None
    disp = g(z['sf_input_disp'])
    valid = c(K.laplacian_valid(disp, disp.max(), 0.03))
    d0 = torch.from_numpy(z['sf_input_disp'])
    want = (oracle.spatial_filter(d0 / d0.max(), 'laplacian').abs() < 0.03).float().numpy()
    assert_bits_equal(valid, want, 'laplacian_valid vs oracle')
    assert (valid != z['sf_valid_disp']).mean() <= 0.002


def test_pconv_epilogue(K, oracle):
    z = load_golden('partial_conv')
    for tag in 'abc':
        cin, cout, k, s, p = [int(v) for v in z['cfg_' + tag]]
        x, m = torch.from_numpy(z['x_' + tag]), torch.from_numpy(z['m_' + tag])
        raw = torch.nn.functional.conv2d(x * m, torch.from_numpy(z['w_' + tag]), torch.from_numpy(z['b_' + tag]), stride=s, padding=p)
        out, um = K.pconv_epilogue(raw.cuda(), g(z['b_' + tag]), m.cuda(), k, s, p)
        o0, u0 = oracle.pconv_epilogue(raw, torch.from_numpy(z['b_' + tag]), m, k, s, p)
        assert_bits_equal(c(out), o0.numpy(), 'pconv out vs oracle')
        assert_bits_equal(c(um), u0.numpy(), 'pconv mask vs oracle')
        assert_bits_equal(c(um.expand(-1, cout, -1, -1)), z['mask_' + tag], 'update_mask vs reference')


def test_pconv_epilogue_with_its_neighbours_fused_and_prelu_mask(K):
    """What follows a partial-convolution layer inside the GridNet's blocks, fused into the epilogue's pass (kbe_pconv_epilogue's
    prelu_slope / residual) and the block's first activation with the layer's `input * mask_in` (kbe_prelu_mask), against the
    same steps as separate torch operations: bit for bit (each step is one fp32 operation per element either way)."""
    z = load_golden('partial_conv')
    gen = torch.Generator().manual_seed(3)
    for tag in 'abc':
        cin, cout, k, s, p = [int(v) for v in z['cfg_' + tag]]
        x, m = torch.from_numpy(z['x_' + tag]), torch.from_numpy(z['m_' + tag])
        bias = g(z['b_' + tag])
        raw = torch.nn.functional.conv2d(x * m, torch.from_numpy(z['w_' + tag]), torch.from_numpy(z['b_' + tag]), stride=s, padding=p).cuda()
        plain, um = K.pconv_epilogue(raw, bias, m.cuda(), k, s, p)
        slope = (torch.rand(cout, generator=gen) * 0.5 - 0.1).cuda()
        res = torch.randn(raw.shape, generator=gen).cuda()
        act, um2 = K.pconv_epilogue(raw, bias, m.cuda(), k, s, p, act_slope=slope)
        assert torch.equal(um, um2)
        assert_bits_equal(c(act), c(torch.nn.functional.prelu(plain, slope)), 'epilogue + PReLU')
        added, _ = K.pconv_epilogue(raw, bias, m.cuda(), k, s, p, residual=res)
        assert_bits_equal(c(added), c(plain + res), 'epilogue + residual')
        both, _ = K.pconv_epilogue(raw, bias, m.cuda(), k, s, p, act_slope=slope, residual=res)
        assert_bits_equal(c(both), c(torch.nn.functional.prelu(plain + res, slope)), 'epilogue + residual + PReLU')
        # the convolution run without its bias, the epilogue adding it first: what the separate broadcasting add would have made
        raw_nb = torch.nn.functional.conv2d(x * m, torch.from_numpy(z['w_' + tag]), None, stride=s, padding=p).cuda()
        late, um3 = K.pconv_epilogue(raw_nb, bias, m.cuda(), k, s, p, act_slope=slope, residual=res, raw_without_bias=True)
        early, _ = K.pconv_epilogue(raw_nb + bias.view(1, -1, 1, 1), bias, m.cuda(), k, s, p, act_slope=slope, residual=res)
        assert torch.equal(um, um3)
        assert_bits_equal(c(late), c(early), 'epilogue adding the bias itself')
        # the block's first activation and the mask multiplication: masks of one channel (how the GridNet carries them)
        sl_in = (torch.rand(cin, generator=gen) * 0.5 - 0.1).cuda()
        m1 = m[:, :1].contiguous().cuda()
        assert_bits_equal(c(K.prelu_mask(x.cuda(), sl_in, m1)), c(torch.nn.functional.prelu(x.cuda(), sl_in) * m1), 'prelu * mask')
        assert_bits_equal(c(K.prelu_mask(x.cuda(), sl_in, None)), c(torch.nn.functional.prelu(x.cuda(), sl_in)), 'prelu alone')


def test_bias_act_and_upsample_act_against_the_separate_torch_passes(K):
    """kbe_bias_act: the bias add, the PReLU and up to two residual adds behind a convolution of the plain networks in one pass --
    against the same steps as separate torch operations, bit for bit (each is one fp32 operation per element either way), with
    every combination of operands, a pixel count that is a multiple of four (vector path) and one that is not.
    kbe_upsample2x_act: bilinear x2 (align_corners=False) + PReLU against F.interpolate + F.prelu: PyTorch's kernel is built with
    contraction to fused multiply-adds, this one is not -- a few units in the last place of the blend; odd sizes and one-pixel
    borders included."""
    F = torch.nn.functional
    gen = torch.Generator().manual_seed(17)
    for (B, C, H, W) in [(1, 5, 12, 20), (2, 3, 7, 9), (1, 64, 33, 47), (1, 1, 1, 1)]:
        x = torch.randn(B, C, H, W, generator=gen).cuda()
        bias, slope = torch.randn(C, generator=gen).cuda(), (torch.rand(C, generator=gen) * 0.5 - 0.1).cuda()
        r1, r2 = torch.randn(B, C, H, W, generator=gen).cuda(), torch.randn(B, C, H, W, generator=gen).cuda()
        for use_b in (False, True):
            for use_s in (False, True):
                for n_res in (0, 1, 2):
                    want = x + bias.view(1, -1, 1, 1) if use_b else x
                    want = F.prelu(want, slope) if use_s else want
                    want = want + r1 if n_res >= 1 else want
                    want = want + r2 if n_res >= 2 else want
                    got = K.bias_act(x, bias if use_b else None, slope if use_s else None, r1 if n_res >= 1 else None, r2 if n_res >= 2 else None)
                    assert_bits_equal(c(got), c(want), 'bias_act %s bias=%s slope=%s residuals=%d' % ((B, C, H, W), use_b, use_s, n_res))
        y = x.clone()
        assert K.bias_act(y, bias, slope, r1, out=y).data_ptr() == y.data_ptr()
        assert_bits_equal(c(y), c(F.prelu(x + bias.view(1, -1, 1, 1), slope) + r1), 'bias_act in place')
        for sl in (slope, None):
            up = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
            want = F.prelu(up, sl) if sl is not None else up
            got = K.upsample2x_act(x, sl)
            assert got.shape == (B, C, 2 * H, 2 * W)
            err = float((got - want).abs().max())
            assert err <= 4e-7 * max(1.0, float(x.abs().max())), 'upsample2x_act %s: %.3g' % ((B, C, H, W), err)


def test_crop_resize_matches_written_algorithm(K, oracle):
    rng = np.random.default_rng(5)
    # even / odd crops (sub-pixel 0.5 and 0), the full frame (replicated border taps), widths that are not a
    # multiple of 4 or of the 64 x 8 tile, tiny crops (every output pixel blends the same few patch pixels), 1024^2
    for (H, W, cw, ch) in [(48, 64, 57, 43), (48, 64, 58, 44), (96, 128, 115, 86), (33, 47, 47, 33), (64, 64, 64, 64),
                           (130, 258, 3, 2), (71, 193, 192, 70), (9, 5, 4, 7), (256, 1024, 900, 225), (1024, 1024, 819, 819)]:
        f = (rng.random((H, W, 3)) * 255).astype(np.uint8)
        out = c(K.crop_resize_u8(torch.from_numpy(f).cuda(), cw, ch))
        assert np.array_equal(out, oracle.crop_resize_u8(f, cw, ch))


def test_crop_resize_properties_at_full_sizes(K):
    """Size-independent properties of getRectSubPix + resize on the device at BASELINE's frame sizes (the oracle is compared at 1024^2
    above; 2048^2 takes it minutes): a constant frame stays that constant (both steps' weights sum to one and every rounding is exact
    on equal taps), a two-valued frame stays within its two values, and the result does not depend on what lies outside the window
    the crop reads (common.crop_window: the rectangle kbe_render_video fills holes in)."""
    from ken_burns_effect_amd import common
    g = torch.Generator(device='cuda').manual_seed(11)
    for (H, W, cw, ch) in [(1024, 1024, 921, 921), (1024, 1024, 920, 920), (2048, 2048, 1843, 1843), (2048, 2048, 1740, 1741), (1080, 1920, 1728, 972), (333, 517, 401, 299)]:
        for v in (0, 1, 127, 255):
            out = K.crop_resize_u8(torch.full((H, W, 3), v, dtype=torch.uint8, device='cuda'), cw, ch)
            assert out.shape == (H, W, 3) and bool((out == v).all()), (H, W, cw, ch, v)
        two = (torch.rand(H, W, 3, device='cuda', generator=g) > 0.5).to(torch.uint8) * 200 + 20
        out = K.crop_resize_u8(two, cw, ch)
        assert int(out.min()) >= 20 and int(out.max()) <= 220, (H, W, cw, ch)
        x0, y0, x1, y1 = common.crop_window(W, H, cw, ch)
        noise = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device='cuda', generator=g)
        other = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device='cuda', generator=g)
        other[y0:y1 + 1, x0:x1 + 1] = noise[y0:y1 + 1, x0:x1 + 1]
        assert torch.equal(K.crop_resize_u8(noise, cw, ch), K.crop_resize_u8(other, cw, ch)), (H, W, cw, ch)


# ---------------------------------------------------------------------------------------
# whole frames
# ---------------------------------------------------------------------------------------

def _scene(size, seed=0, kind='smooth', dolly=False):
    from ken_burns_effect_amd import common, synthetic
    image, disp = synthetic.make_rgbd(size[0], size[1], seed, kind)
    depth = (512.0 * 120) / (disp + 1e-7)
    Kn = common._K()
    oc = {'dblFocal': 512.0, 'dblBaseline': 120, 'intWidth': size[1], 'intHeight': size[0],
          'objectDepthrange': synthetic.depthrange_of(depth), 'tensorRawImage': image.cuda(),
          'tensorRawDisparity': disp.cuda(), 'tensorRawDepth': depth.cuda()}
    oc['tensorRawPoints'] = Kn.depth_to_points(oc['tensorRawDepth'], 512.0).view(1, 3, -1)
    common._reset_inpa(oc)
    ofrom, oto = synthetic.default_windows(size[0], size[1], dolly)
    settings = {'dblSteps': [0.0, 0.5, 1.0], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': dolly,
                'boolCrop': False}
    return settings, oc


@pytest.mark.parametrize('size,kind,dolly', [((96, 128), 'smooth', False), ((256, 256), 'smooth', True),
                                              ((200, 312), 'noise', False), ((512, 512), 'smooth', False)])
def test_frames_match_oracle(K, oracle, size, kind, dolly):
    from ken_burns_effect_amd import common
    settings, oc = _scene(size, 3, kind, dolly)
    cams = common.frame_cameras(settings, oc)
    frames = common.render_frames(cams, oc, None)
    ok = oracle.OracleKernels('jacobi')
    state = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), size[1], size[0])
    src = (oc['tensorRawImage'][0].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)
    hip_state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], size[1], size[0])
    for f, (focal, shift3) in zip(frames, cams):
        ref, ref_float, ref_existing = ok.render_frame(state, shift3, focal, oc['dblBaseline'], want_float=True)
        ref = ref.numpy()
        # uint8 truncation can flip a value sitting on an integer boundary by one count
        d = np.abs(f.astype(np.int32) - ref.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
        # "within 1e-3 PSNR": both frames score the same against any third image
        assert abs(psnr(f, src, 255.0) - psnr(ref, src, 255.0)) < 1e-3
        # the float render behind the frame
        rf = torch.empty(4, size[0], size[1], device='cuda')
        ex = torch.empty(size[0] * size[1], device='cuda')
        zd, zp = torch.empty_like(ex), torch.empty_like(ex)
        f2 = K.render_frame(hip_state, shift3, focal, oc['dblBaseline'], render_f32=rf, existing_f32=ex, zee_f32=zd, zee_pre_f32=zp)
        d2 = np.abs(c(f2).astype(np.int32) - f.astype(np.int32))      # two runs differ only by atomic summation order
        assert d2.max() <= 1 and (d2 > 0).mean() < 1e-3, 'debug outputs do not change the frame'
        assert np.array_equal(c(ex).reshape(size) > 0, ref_existing.numpy()[0, 0] > 0), 'same holes'
        assert psnr(c(rf)[:3], ref_float.numpy()[0, :3], 1.0) > 100.0
        # z-buffer of the tiled path: bit-exact against the oracle, before and after degrid
        pts = oracle.shift_points(state['points'], torch.tensor(shift3))
        z0, _ = oracle.zsplat(pts, size[1], size[0], focal, oc['dblBaseline'])
        assert_bits_equal(c(zp).reshape(size), z0.numpy()[0, 0], 'tile z-buffer (pre-degrid)')
        assert_bits_equal(c(zd).reshape(size), oracle.degrid(z0, 'jacobi').numpy()[0, 0], 'tile z-buffer (degridded)')


def test_full_size_zbuffer_is_the_min_over_winners(K):
    """1024x1024 (BASELINE.json size): the z-buffer must equal an independent scatter-min of
    dblError over each point's winner pixel (torch, fp64 -> fp32), bit for bit."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((1024, 1024), 0)
    focal, shift3 = common.frame_cameras(settings, oc)[2]
    pts = oc['tensorInpaPoints']
    zkeys, winner = K.zsplat(pts, 1024, 1024, focal, 120, shift3=shift3, want_winner=True)
    zee = K.zkeys_decode(zkeys).view(-1)
    shifted = K.shift_points(pts, shift3)
    err = (1000000.0 - (focal * 120) / (shifted[0, 2].double() + 0.0000001)).float()
    w = winner[0].long()
    keep = w >= 0
    want = torch.full((1024 * 1024,), 1000000.0, device='cuda')
    want.scatter_reduce_(0, w[keep], err[keep], reduce='amin')
    assert torch.equal(zee.view(torch.int32), want.view(torch.int32))
    assert int(keep.sum()) > 900000


def test_full_size_identity_camera_reproduces_the_image(K):
    """No shift, same focal: every point lands on its own pixel -> the frame is the source image."""
    settings, oc = _scene((1024, 1024), 1)
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], 1024, 1024)
    rf = torch.empty(4, 1024, 1024, device='cuda')
    ex = torch.empty(1024 * 1024, device='cuda')
    K.render_frame(state, [0.0, 0.0, 0.0], 512.0, 120, render_f32=rf, existing_f32=ex)
    assert float((ex > 0).float().mean()) == 1.0
    assert float((rf[:3] - oc['tensorRawImage'][0]).abs().max()) < 1e-3


def test_full_size_linearity_in_the_data(K):
    """accumulate + normalise are linear in the data channels (size-independent property)."""
    settings, oc = _scene((1024, 1024), 2)
    from ken_burns_effect_amd import common
    focal, shift3 = common.frame_cameras(settings, oc)[1]
    pts = K.shift_points(oc['tensorInpaPoints'], shift3)
    d1 = oc['tensorInpaImage']
    d2 = torch.rand_like(d1)
    ra, _ = K.render_pointcloud(pts, d1, 1024, 1024, focal, 120)
    rb, _ = K.render_pointcloud(pts, d2, 1024, 1024, focal, 120)
    rc, _ = K.render_pointcloud(pts, 0.25 * d1 + 2.0 * d2, 1024, 1024, focal, 120)
    assert float((rc - (0.25 * ra + 2.0 * rb)).abs().max()) < 1e-4


def test_cropped_frames_ignore_holes_outside_the_crop(K, oracle):
    """process_kenburns with the crop of common.py:256-257: the HIP path fills only the holes inside the
    crop window; the oracle fills all of them and then crops.  The cropped frames must agree."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((192, 256), 7)
    settings.pop('boolCrop')
    frames = common.process_kenburns(dict(settings, boolInpaint=False), oc, None)
    ok = oracle.OracleKernels('jacobi')
    state = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), 256, 192)
    cw, ch = common.crop_size(settings)
    for f, (focal, shift3) in zip(frames, common.frame_cameras(settings, oc)):
        ref = oracle.crop_resize_u8(ok.render_frame(state, shift3, focal, oc['dblBaseline']).numpy(), cw, ch)
        # (HIP against the oracle through the crop: the raw frames differ by one count on a few values -- the order of the fp32
        # sums -- and one count at one raw value moves a CROPPED value by up to two in rare places, through the fixed-point
        # getRectSubPix + resize: frames_close's `cropped` bound, found in round 4 by perturbing a raw frame value by value)
        d = np.abs(f.astype(np.int32) - ref.astype(np.int32))
        assert d.max() <= 2 and (d > 0).mean() < 2e-3 and (d > 1).mean() < 1e-5, 'max %d, %.2e differ, %.2e by more than one' % (d.max(), (d > 0).mean(), (d > 1).mean())


def test_native_frame_loop_equals_per_frame_calls(K):
    """kbe_render_video (frames + crop + overlapped copies enqueued from C) against one call per frame."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((160, 224), 8)
    settings = dict(settings, dblSteps=[i / 6.0 for i in range(7)])
    cams = common.frame_cameras(settings, oc)
    crop = common.crop_size(settings)
    a = common.render_frames(cams, oc, crop)                               # native loop, pinned host memory
    state = common._prepared_cloud(K, oc)
    rect = common.crop_window(224, 160, crop[0], crop[1])
    b = np.stack([K.crop_resize_u8(K.render_frame(state, sh, f, oc['dblBaseline'], fill_rect=rect), crop[0], crop[1]).cpu().numpy()
                  for f, sh in cams])                                      # one C call per kernel sequence
    dev = common.render_frames(cams, oc, crop, keep_on_device=True)        # native loop, frames left in HBM
    assert dev.is_cuda and a.shape == b.shape == tuple(dev.shape) == (7, 160, 224, 3)
    for other in (b, dev.cpu().numpy()):
        frames_close(a, other, 'cropped frames', cropped=True)
    c2 = common.render_frames(cams, oc, None)
    assert c2.shape == (7, 160, 224, 3)
    # every hand-off to pinned host memory delivers the same bytes: groups of frames per runtime transfer with the lanes
    # taking turns (default; here explicit group sizes incl. a ragged last group), the per-frame copy kernel, and
    # round 1's staged ring
    for batch in (-1, -2, -3, 0, 3):
        other = common.render_frames(cams, oc, crop, batch=batch)
        assert np.array_equal(other, a), 'hand-off batch=%d' % batch


@pytest.mark.parametrize('lanes', ['1', '2', '4'])
@pytest.mark.parametrize('n_frames', [1, 2, 5, 8])
def test_bucket_route_video_alternates_its_z_buffers(K, monkeypatch, lanes, n_frames):
    """On the bucket route consecutive frames of a lane alternate between two z-buffers, each frame's tile launch
    clearing the other's (no reset pass); whatever the number of frames and lanes, every frame must equal the frame
    rendered on its own, and a stand-alone frame rendered AFTER the video must find its z-buffer empty."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', '0')
    monkeypatch.setenv('KBE_LANES', lanes)
    settings, oc = _scene((160, 224), 8)
    settings = dict(settings, dblSteps=[i / max(n_frames - 1, 1) for i in range(n_frames)])
    cams = common.frame_cameras(settings, oc)
    state = common._prepared_cloud(K, oc)
    assert not state['fused']
    alone = np.stack([K.render_frame(state, sh, f, oc['dblBaseline']).cpu().numpy() for f, sh in cams])
    for _ in range(2):                                                      # twice: the second video starts from the first one's leftovers
        video = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
        d = np.abs(video.astype(np.int32) - alone.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
        again = K.render_frame(state, cams[0][1], cams[0][0], oc['dblBaseline']).cpu().numpy()
        d = np.abs(again.astype(np.int32) - alone[0].astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
    # the flags by hand: A, B, A, B then a stand-alone frame
    zp = torch.empty(160 * 224, device='cuda')
    ref = torch.empty_like(zp)
    K.render_frame(state, cams[-1][1], cams[-1][0], oc['dblBaseline'], zee_pre_f32=ref, stages=7)
    for k in range(4):
        K.render_frame(state, cams[-1][1], cams[-1][0], oc['dblBaseline'], zee_pre_f32=zp, stages=7 | (256 if k & 1 else 128))
        assert torch.equal(zp.view(torch.int32), ref.view(torch.int32)), 'z-buffer of alternating frame %d' % k
    K.render_frame(state, cams[-1][1], cams[-1][0], oc['dblBaseline'], zee_pre_f32=zp, stages=7)
    assert torch.equal(zp.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize('host_lanes', ['2', '3', '4'])
@pytest.mark.parametrize('batch,n_frames', [(-2, 16), (-4, 19), (-8, 32), (-4, 16), (-8, 19), (-16, 64)])
def test_bucket_route_video_delivered_in_groups_alternates_its_z_buffers(K, monkeypatch, host_lanes, batch, n_frames):
    """Frames handed to pinned host memory in groups of G = -batch per lane, ONE frame per launch (the shape of the 1024^2
    bench): a lane then renders whole groups of consecutive frames, so its last frame is not `i + lanes >= n_frames`.
    (Round 2 got that wrong: frames in the middle of a lane's share ran stand-alone, left z-buffer B dirty, and the lane's
    next B frame rendered over stale keys -- lanes=2, n=64, G=8 -> frame 63.)  Every delivered frame must equal the frame
    rendered on its own, twice in a row, and a stand-alone frame afterwards must find an empty z-buffer."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', '0')
    monkeypatch.setenv('KBE_FILL_GROUP', '1')
    monkeypatch.setenv('KBE_LANES', '4')
    monkeypatch.setenv('KBE_HOST_LANES', host_lanes)
    settings, oc = _scene((160, 224), 8)
    settings = dict(settings, dblSteps=[i / (n_frames - 1) for i in range(n_frames)])
    cams = common.frame_cameras(settings, oc)
    state = common._prepared_cloud(K, oc)
    assert not state['fused']
    alone = np.stack([K.render_frame(state, sh, f, oc['dblBaseline']).cpu().numpy() for f, sh in cams])
    for rep in range(2):
        video = common.render_frames(cams, oc, None, batch=batch)
        d = np.abs(video.astype(np.int32) - alone.astype(np.int32))
        worst = [int(i) for i in np.nonzero(d.reshape(n_frames, -1).max(axis=1) > 1)[0]]
        assert not worst, 'pass %d: frames %s differ from the frames rendered on their own' % (rep, worst)
        assert (d > 0).mean() < 1e-3
        again = K.render_frame(state, cams[0][1], cams[0][0], oc['dblBaseline']).cpu().numpy()
        d = np.abs(again.astype(np.int32) - alone[0].astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, 'a stand-alone frame after the video (pass %d)' % rep


def test_group_of_frames_per_launch_equals_frames_on_their_own(K, monkeypatch):
    """kbe_render_frame_group: projection, tile and fill launches that take 1..4 frames each (one grid dimension is the
    frame), every frame with its own camera and scratch set, against kbe_render_frame per frame -- twice, the second time
    with the sets' z-buffers alternating (A, then B)."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', '0')
    settings, oc = _scene((200, 312), 4, 'noise')
    settings = dict(settings, dblSteps=[0.0, 0.3, 0.7, 1.0])
    cams = common.frame_cameras(settings, oc)
    state = common._prepared_cloud(K, oc)
    alone = torch.stack([K.render_frame(state, sh, f, oc['dblBaseline']).clone() for f, sh in cams])
    for n in (1, 3, 4):
        out = torch.zeros(n, 200, 312, 3, dtype=torch.uint8, device='cuda')
        for flags in (None, [128] * n, [256] * n, None):
            out.zero_()
            K.render_frame_group(state, cams[:n], oc['dblBaseline'], out, zbuf_flags=flags)
            d = (out.int() - alone[:n].int()).abs()
            assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 1e-3, 'n=%d flags=%s' % (n, flags)
    with pytest.raises(Exception):
        K.render_frame_group(state, cams * 2, oc['dblBaseline'], torch.zeros(8, 200, 312, 3, dtype=torch.uint8, device='cuda'))


@pytest.mark.parametrize('fused', ['0', '1'])
@pytest.mark.parametrize('group,n_frames,lanes', [('2', 7, '4'), ('3', 13, '2'), ('4', 16, '4'), ('4', 5, '3'), ('2', 1, '2')])
def test_video_that_fills_several_frames_per_launch_equals_frames_on_their_own(K, monkeypatch, fused, group, n_frames, lanes):
    """KBE_VIDEO_FILL_GROUP(n): a lane scatters n frames into n scratch sets and fills them in the same launches (dolly
    zooms with the table-driven fill).  Every frame must equal the frame rendered on its own (within the accumulation order) -- whole groups, ragged last
    groups, a single frame; both scatter routes (the bucket route's sets alternate their z-buffers separately, the fused
    route's their hole counters); frames left in HBM and delivered to host memory, cropped and not; twice in a row."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', fused)
    monkeypatch.setenv('KBE_LANES', lanes)
    monkeypatch.setenv('KBE_FILL_DIST', '1')
    monkeypatch.setenv('KBE_FILL_GROUP', group)
    size = (384, 416)
    settings, oc = _scene(size, 11, 'smooth', True)
    settings = dict(settings, dblSteps=[i / max(n_frames - 1, 1) for i in range(n_frames)])
    cams = common.frame_cameras(settings, oc)
    crop = common.crop_size(settings)
    state = common._prepared_cloud(K, oc)
    assert state['fused'] == (fused == '1')
    def same(a, b, what=''):
        # the colour sums depend on the order records reach a bucket (last ulp): a uint8 value on an integer boundary may flip
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, '%s: max %d, %.2e of the values differ' % (what, d.max(), (d > 0).mean())

    alone = np.stack([K.render_frame(state, sh, f, oc['dblBaseline']).cpu().numpy() for f, sh in cams])
    assert n_frames < 5 or int((alone[-1] == 0).all(axis=2).sum()) > 49152, 'late frames have enough holes for the table-driven schedule'
    for _ in range(2):
        video = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
        same(video, alone, 'frames left in HBM')
        same(common.render_frames(cams, oc, None), alone, 'delivered to host memory')
    rect = common.crop_window(size[1], size[0], crop[0], crop[1])
    cropped = np.stack([K.crop_resize_u8(K.render_frame(state, sh, f, oc['dblBaseline'], fill_rect=rect), crop[0], crop[1]).cpu().numpy() for f, sh in cams])
    frames_close(common.render_frames(cams, oc, crop), cropped, 'cropped', cropped=True)
    monkeypatch.setenv('KBE_FILL_GROUP', '1')
    same(common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy(), alone, 'one frame per launch')
    again = K.render_frame(state, cams[0][1], cams[0][0], oc['dblBaseline']).cpu().numpy()       # the scratch of lane 0 is as a video leaves it
    same(again, alone[0], 'a frame on its own after the videos')


def test_pipelined_groups_equal_groups_with_their_placements_in_front(K):
    """kbe_render_frame_group_ahead: the tile launch of a group makes the placements of the NEXT group (the other bank of the
    sets' placements, lists and counters; list totals rotating over three words).  A sequence of groups of changing sizes --
    ramping up, a set sitting out, a lone frame, twelve frames -- renders the frames of the same groups with their placement
    launches in front (within the accumulation order), and leaves the sets clean for frames on their own."""
    from ken_burns_effect_amd import common
    size = (200, 312)
    settings, oc = _scene(size, 21, 'smooth', True)
    settings = dict(settings, dblSteps=[i / 39 for i in range(40)])
    cams = common.frame_cameras(settings, oc)
    state = common._prepared_cloud(K, oc)
    K._pack(state)
    Bl = oc['dblBaseline']
    sizes = [1, 2, 4, 3, 12, 1, 5]
    groups, at = [], 0
    for n in sizes:
        groups.append([cams[(at + k) % len(cams)] for k in range(n)])
        at += n
    want = []
    for g in groups:
        buf = torch.zeros(len(g), size[0], size[1], 3, dtype=torch.uint8, device='cuda')
        K.render_frame_group_fused(state, g, Bl, buf)
        want.append(buf.cpu().numpy())
    for rep in range(2):
        turns = [0] * 12                    # per scratch set: how often the sequence has used it
        placed = False
        for i, g in enumerate(groups):
            n = len(g)
            nxt = groups[i + 1] if i + 1 < len(groups) else None
            ok = nxt is not None and bool(K.lib.kbe_render_frame_group_ahead_ok(state['N'], size[1], size[0], n, len(nxt)))
            now = turns[:n]
            for k in range(n):
                turns[k] += 1
            buf = torch.zeros(n, size[0], size[1], 3, dtype=torch.uint8, device='cuda')
            K.render_frame_group_ahead(state, g, Bl, buf, turn=now, placed=placed, next_cameras=nxt if ok else None, next_turn=turns[:len(nxt)] if ok else None)
            placed = ok
            d = np.abs(buf.cpu().numpy().astype(np.int32) - want[i].astype(np.int32))
            assert d.max() <= 1 and (d > 0).mean() < 1e-3, 'pass %d group %d (%d frames): max %d, %.2e differ' % (rep, i, n, d.max(), (d > 0).mean())
        # the sets are clean: frames on their own (parity -1 zeroes the counters; the banks must be empty)
        buf = torch.zeros(12, size[0], size[1], 3, dtype=torch.uint8, device='cuda')
        K.render_frame_group_fused(state, groups[4], Bl, buf)
        d = np.abs(buf.cpu().numpy().astype(np.int32) - want[4].astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
    with pytest.raises(Exception):          # a set used by both groups must take consecutive turns
        K.render_frame_group_ahead(state, groups[1], Bl, torch.zeros(2, size[0], size[1], 3, dtype=torch.uint8, device='cuda'), turn=[0, 0], placed=False,
                                   next_cameras=groups[1], next_turn=[1, 2])


def test_a_fused_group_with_a_bad_frame_enqueues_nothing(K):
    """kbe_render_frame_group_fused checks every frame before it enqueues anything: a misaligned scratch set in the second frame is
    refused, and the first frame's set -- parity -1, whose hole counters the call would zero first -- is left as it was."""
    import ctypes
    from ken_burns_effect_amd import common
    size = (96, 128)
    settings, oc = _scene(size, 5)
    cams = common.frame_cameras(settings, oc)[:2]
    state = common._prepared_cloud(K, oc)
    K._pack(state)
    stride = K.scratch_stride(state)
    scratch = torch.full((2 * stride,), 0xAB, dtype=torch.uint8, device='cuda')
    out = torch.zeros(2, size[0], size[1], 3, dtype=torch.uint8, device='cuda')
    focals = (ctypes.c_double * 2)(*[float(c[0]) for c in cams])
    shifts = (ctypes.c_float * 6)(*[float(v) for c in cams for v in c[1]])
    sets = (ctypes.c_void_p * 2)(scratch.data_ptr(), scratch.data_ptr() + stride + 8)
    frames = (ctypes.c_void_p * 2)(out[0].data_ptr(), out[1].data_ptr())
    rc = K.lib.kbe_render_frame_group_fused(ctypes.c_void_p(state['packed'].data_ptr()), state['N'], ctypes.c_double(state['cloud_focal']), size[1], size[0],
                                            ctypes.c_double(oc['dblBaseline']), 2, focals, shifts, sets, frames, None, 6, None,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and b'bad scratch' in K.lib.kbe_last_error()
    assert bool((scratch == 0xAB).all()), 'the first frame\'s set was written before the second frame was checked'


@pytest.mark.parametrize('kind', ['incoherent', 'pile_up', 'tiny', 'empty'])
def test_pipelined_groups_through_the_slow_paths(K, kind):
    """The one-launch scatter on clouds that leave the normal path: a cloud in random order (every sub-block is wide: the list
    totals -- which rotate over three words in a pipelined sequence -- exceed their budget and every tile scans the cloud), four
    points per pixel (records spill), a 37 x 50 frame (partial tiles, fewer tiles than waves have units), no points at all.
    Five groups of changing size, pipelined, against the same groups with their placement launches in front."""
    g0 = torch.Generator().manual_seed(11)
    if kind == 'incoherent':
        W, H, N = 200, 136, 6000
        pts = torch.rand(1, 3, N, generator=g0) * torch.tensor([1600.0, 1200.0, 900.0]).view(1, 3, 1) - torch.tensor([800.0, 600.0, -100.0]).view(1, 3, 1)
        pts[0, 2, :50] = 0.0
        pts[0, 2, 50:100] = -30.0
    elif kind == 'pile_up':
        W, H = 96, 64
        N = 4 * W * H
        u = torch.rand(N, generator=g0) * (W + 8) - 4 - W / 2 + 0.5
        v = torch.rand(N, generator=g0) * (H + 8) - 4 - H / 2 + 0.5
        z = torch.rand(N, generator=g0) * 400 + 600
        pts = torch.stack([u * z / 512.0, v * z / 512.0, z]).unsqueeze(0)
    elif kind == 'tiny':
        W, H, N = 50, 37, 50 * 37
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
        z = 700.0 + 200.0 * torch.rand(H, W, generator=g0)
        pts = torch.stack([(xs - W / 2 + 0.5) * z / 512.0, (ys - H / 2 + 0.5) * z / 512.0, z]).reshape(1, 3, -1)
    else:
        W, H, N = 64, 48, 0
        pts = torch.zeros(1, 3, 0)
    img, dep = torch.rand(1, 3, N, generator=g0), torch.rand(1, 1, N, generator=g0) * 500 + 100
    state = K.prepare_cloud(pts.cuda(), img.cuda(), dep.cuda(), W, H)
    K._pack(state)
    cams = [(512.0 - 6.0 * i, (1.5 * i - 4.0, 2.0 - 0.7 * i, -3.0 * i)) for i in range(14)]
    sizes = [2, 3, 3, 1, 5]
    groups, at = [], 0
    for n in sizes:
        groups.append(cams[at:at + n])
        at += n
    want = []
    for g in groups:
        buf = torch.zeros(len(g), H, W, 3, dtype=torch.uint8, device='cuda')
        K.render_frame_group_fused(state, g, 120, buf)
        want.append(c(buf))
    for rep in range(2):
        turns, placed = [0] * 12, False
        for i, g in enumerate(groups):
            n = len(g)
            nxt = groups[i + 1] if i + 1 < len(groups) else None
            ok = nxt is not None and bool(K.lib.kbe_render_frame_group_ahead_ok(N, W, H, n, len(nxt)))
            now = turns[:n]
            for k in range(n):
                turns[k] += 1
            buf = torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
            K.render_frame_group_ahead(state, g, 120, buf, turn=now, placed=placed, next_cameras=nxt if ok else None, next_turn=turns[:len(nxt)] if ok else None)
            placed = ok
            d = np.abs(c(buf).astype(np.int32) - want[i].astype(np.int32))
            assert d.max() <= 1 and (d > 0).mean() < 2e-3, '%s, pass %d group %d: max %d, %.2e differ' % (kind, rep, i, d.max(), (d > 0).mean())
    assert kind == 'empty' or any(w.any() for w in want), 'the frames show something'


@pytest.mark.parametrize('density', [1, 2])
def test_lean_and_roomy_builds_of_the_tile_launch_render_the_same_frames(K, monkeypatch, density):
    """Every tile launch of the fused route exists twice (kbe_fused.hip): LEAN -- 608 records per tile in LDS, six workgroups per
    CU, what clouds of about a point per pixel take -- and ROOMY (736, five).  KBE_FUSED_CAP forces either: the same groups,
    pipelined and with their placement launches in front, on a cloud of one point per pixel (whose tiles hold about as many
    records as the lean build has room for: many of them spill a few and take a second round) and on one of two per pixel (every
    tile spills on either build)."""
    g0 = torch.Generator().manual_seed(9)
    W, H = 192, 128
    n_side = density
    ys, xs = torch.meshgrid(torch.arange(H * n_side, dtype=torch.float32) / n_side, torch.arange(W, dtype=torch.float32), indexing='ij')
    z = 500.0 + 300.0 * torch.rand(ys.shape, generator=g0)
    pts = torch.stack([(xs - W / 2 + 0.5) * z / 512.0, (ys - H / 2 + 0.5) * z / 512.0, z]).reshape(1, 3, -1)
    N = pts.shape[2]
    img, dep = torch.rand(1, 3, N, generator=g0), torch.rand(1, 1, N, generator=g0) * 500 + 100
    monkeypatch.setenv('KBE_FUSED', '1')
    state = K.prepare_cloud(pts.cuda(), img.cuda(), dep.cuda(), W, H)
    K._pack(state)
    cams = [(512.0, (0.4 * i - 2.0, 1.0 - 0.2 * i, -1.5 * i)) for i in range(10)]
    groups = [cams[0:4], cams[4:9], cams[9:10]]
    frames = {}
    for build in ('lean', 'roomy'):
        monkeypatch.setenv('KBE_FUSED_CAP', build)
        got = []
        for g in groups:
            buf = torch.zeros(len(g), H, W, 3, dtype=torch.uint8, device='cuda')
            K.render_frame_group_fused(state, g, 120, buf)
            got.append(c(buf))
        turns, placed = [0] * 12, False
        for i, g in enumerate(groups):
            n = len(g)
            nxt = groups[i + 1] if i + 1 < len(groups) else None
            ok = nxt is not None and bool(K.lib.kbe_render_frame_group_ahead_ok(N, W, H, n, len(nxt)))
            now = turns[:n]
            for k in range(n):
                turns[k] += 1
            buf = torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
            K.render_frame_group_ahead(state, g, 120, buf, turn=now, placed=placed, next_cameras=nxt if ok else None, next_turn=turns[:len(nxt)] if ok else None)
            placed = ok
            d = np.abs(c(buf).astype(np.int32) - got[i].astype(np.int32))
            assert d.max() <= 1 and (d > 0).mean() < 2e-3, '%s, group %d pipelined: max %d, %.2e differ' % (build, i, d.max(), (d > 0).mean())
        frames[build] = got
    for other in ('roomy',):
        for a, b in zip(frames['lean'], frames[other]):
            d = np.abs(a.astype(np.int32) - b.astype(np.int32))
            assert a.any() and d.max() <= 1 and (d > 0).mean() < 2e-3, 'lean against %s: max %d, %.2e differ' % (other, d.max(), (d > 0).mean())


@pytest.mark.parametrize('build', ['lean', 'roomy', 'no_ahead', 'dense', 'delivered'])
def test_every_instantiation_of_the_tile_launch_against_the_oracle(K, oracle, monkeypatch, build):
    """The tile launch of the fused route is ONE template in nine instantiations (kbe_fused.hip: lean / roomy / dense x a launch that
    places ahead or not x one frame or a group).  The other tests of the group launches compare HIP with HIP; this one holds each
    non-default instantiation against the ORACLE: a 26-frame video at 512 x 512 left in HBM -- twelve frames
    per launch, so k_frame_group_ahead* runs, with k_place in front and k_frame_group* at the end -- every third frame against
    oracle.render_frame on the same cloud (Jacobi schedule): one count on < 0.1 % of the values.  `lean` / `roomy`:
    KBE_FUSED_CAP; `no_ahead`: KBE_AHEAD=0 (k_place + k_frame_group* per group); `dense`: four points per pixel (an upsampled
    cloud: k_frame_group_ahead_dense, colours fetched behind the splat); `delivered`: to pinned host memory, cropped (the ramp's
    groups of 1, 2, 4, ...: k_frame / k_frame_ahead as well)."""
    from ken_burns_effect_amd import common, synthetic
    size = 512
    settings, oc = _scene((size, size), 5)
    monkeypatch.setenv('KBE_FUSED', '1')
    monkeypatch.setenv('KBE_FILL_GROUP', '12')
    monkeypatch.setenv('KBE_LANES', '1')                # one lane: groups of 12, 12, 2 frames follow one another, each launch placing the next group
    if build in ('lean', 'roomy'):
        monkeypatch.setenv('KBE_FUSED_CAP', build)
    if build == 'no_ahead':
        monkeypatch.setenv('KBE_AHEAD', '0')
    if build == 'dense':
        up = 2
        image_u, disp_u = synthetic.make_rgbd(size * up, size * up, 5)
        depth_u = ((512.0 * 120) / (disp_u + 1e-7)).cuda()
        oc['tensorInpaPoints'] = K.depth_to_points(depth_u, 512.0 * up).view(1, 3, -1)
        oc['tensorInpaImage'] = image_u.cuda().reshape(1, 3, -1)
        oc['tensorInpaDepth'] = depth_u.reshape(1, 1, -1)
        oc['_kbeCloudRaster'] = (size * up, size * up * size * up)
    n = 26
    cams = common.frame_cameras(dict(settings, dblSteps=np.linspace(0.0, 1.0, n).tolist()), oc)
    crop = None
    if build == 'delivered':
        crop = common.crop_size(settings)
        frames = common.render_frames(cams, oc, crop)
    else:
        frames = c(common.render_frames(cams, oc, None, keep_on_device=True))
    ok = oracle.OracleKernels('jacobi')
    state = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), size, size)
    for i in range(0, n, 3):
        focal, shift3 = cams[i]
        ref = ok.render_frame(state, shift3, focal, oc['dblBaseline']).numpy()
        if crop is not None:
            ref = oracle.crop_resize_u8(ref, crop[0], crop[1])
        d = np.abs(frames[i].astype(np.int32) - ref.astype(np.int32))
        bound = 2 if crop is not None else 1            # (through the crop's fixed point: frames_close)
        assert ref.any() and d.max() <= bound and (d > 0).mean() < 1e-3 and (d > 1).mean() < 1e-5, \
            '%s, frame %d: max %d, %.2e of the values differ' % (build, i, d.max(), (d > 0).mean())


def test_cloud_of_nine_points_per_pixel_on_all_three_routes_against_the_oracle(K, oracle, monkeypatch):
    """Until round 5 both tile routes fell off a cliff from 5-6 points per pixel on (candidate lists of 512 sub-blocks and spill
    areas of 16-byte records overflowed on the densest tiles, which then scanned the cloud: 13 ms per 1024^2 frame at 9 per pixel).
    Lists of 2048 entries and records spilled as 4-byte point indices let the fused route grow linearly to 20 per pixel (VERDICT r4
    items 5 and 7).  A 3 x 3-upsampled cloud on a 96 x 128 raster: the default route is the fused one, its frames -- left in HBM and
    delivered through the crop -- equal the oracle's within the order of the fp32 sums; so do the bucket route's and those of the
    stage-by-stage atomic kernels run as a video loop (KBE_FUSED=generic)."""
    from ken_burns_effect_amd import _native, common, synthetic
    H, W, up = 96, 128, 3
    settings, oc = _scene((H, W), 6)
    image_u, disp_u = synthetic.make_rgbd(H * up, W * up, 6)
    depth_u = ((512.0 * 120) / (disp_u + 1e-7)).cuda()
    oc['tensorInpaPoints'] = K.depth_to_points(depth_u, 512.0 * up).view(1, 3, -1)
    oc['tensorInpaImage'] = image_u.cuda().reshape(1, 3, -1)
    oc['tensorInpaDepth'] = depth_u.reshape(1, 1, -1)
    oc['_kbeCloudRaster'] = (W * up, W * up * H * up)
    assert oc['tensorInpaPoints'].shape[2] == 9 * H * W <= _native.FUSED_MAX_DENSITY * H * W
    cams = common.frame_cameras(dict(settings, dblSteps=[0.0, 0.3, 0.7, 1.0]), oc)
    state = common._prepared_cloud(K, oc)
    assert state['fused'] and not state['generic']
    crop = common.crop_size(settings)
    in_hbm = c(common.render_frames(cams, oc, None, keep_on_device=True))
    delivered = common.render_frames(cams, oc, crop)
    ok = oracle.OracleKernels('jacobi')
    ostate = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), W, H)
    refs = [ok.render_frame(ostate, shift3, focal, oc['dblBaseline']).numpy() for focal, shift3 in cams]
    for i, ref in enumerate(refs):
        frames_close(in_hbm[i], ref, 'fused route, frame %d' % i)
        frames_close(delivered[i], oracle.crop_resize_u8(ref, crop[0], crop[1]), 'fused route, delivered frame %d' % i, cropped=True)
    assert in_hbm.any()
    for route in ('0', 'generic'):                      # the bucket route (slow at this density, not wrong) and the atomic kernels
        monkeypatch.setenv('KBE_FUSED', route)
        oc.pop('_kbePreparedCloud')
        other = c(common.render_frames(cams, oc, None, keep_on_device=True))
        st = common._prepared_cloud(K, oc)
        assert not st['fused'] and st['generic'] == (route == 'generic')
        for i, ref in enumerate(refs):
            frames_close(other[i], ref, 'KBE_FUSED=%s, frame %d' % (route, i))


@pytest.mark.parametrize('steps', [20, 75, 400])
def test_video_on_a_ken_burns_path_with_shared_lists_equals_the_video_with_lists_per_frame(K, monkeypatch, steps):
    """The candidate lists of consecutive frames are shared in sub-groups whose size follows the nearest point's motion between a
    sub-group's first and last camera (kbe_fused_plan.h share_plan; near_depth = objectDepthrange[0]): on the product's own camera path --
    a parabola in shift space -- with 20 steps (7 px per step at 512^2 scaled: lists per frame), 75 (sub-groups) and 400 (whole
    launches share), one lane so that launches of twelve follow one another: the same frames as with KBE_SHARE_LISTS=0 (near_depth 0:
    every frame its own lists), and as the oracle's for a sample of them.  (That the plan does share on such a path, and in which
    sub-groups, is asserted without a GPU: tests/test_fused_plan.py::test_share_plan_fires_on_a_ken_burns_path.)"""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_LANES', '1')
    monkeypatch.setenv('KBE_FILL_GROUP', '12')
    size = 384
    settings, oc = _scene((size, size), 8)
    n = 38
    start = 0.3
    cams = common.frame_cameras(dict(settings, dblSteps=[start + i / (steps - 1.0) for i in range(n) if start + i / (steps - 1.0) <= 1.0]), oc)
    assert len(cams) >= 13
    shared = c(common.render_frames(cams, oc, None, keep_on_device=True))
    assert common._prepared_cloud(K, oc)['near_depth'] == oc['objectDepthrange'][0] > 0
    monkeypatch.setenv('KBE_SHARE_LISTS', '0')
    own = c(common.render_frames(cams, oc, None, keep_on_device=True))
    for i in range(len(cams)):
        frames_close(shared[i], own[i], '%d-step path, frame %d' % (steps, i))
    assert shared.any()


@pytest.mark.parametrize('kind', ['rough', 'near_plane', 'curved'])
def test_groups_sharing_their_candidate_lists_on_clouds_with_large_parallax(K, kind):
    """Consecutive frames a tile launch places ahead share candidate lists in sub-groups (same focal length, shifts only differ:
    kbe_fused.hip, launch_frames_fused's share_plan): a sub-block is listed for the box of its corners under the sub-group's first
    and last camera, widened by how far the cameras in between stray from that chord ('curved': a parabola in shift space, what a
    Ken Burns path is).  On clouds where that box is large or has no bound -- a depth map of
    noise between 3 and 900 under a camera that moves by whole tiles per group ('rough'), and rows of points that pass the near
    plane INSIDE a group ('near_plane': z between 0.5 and 40, the camera advancing by 4 per frame) -- groups of 12, 5, 12, 2
    frames, pipelined, render the frames of the same groups with their per-frame lists (placement launches in front)."""
    g0 = torch.Generator().manual_seed(5)
    W, H = 160, 120
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    z = 3.0 + 897.0 * torch.rand(H, W, generator=g0) ** 2
    if kind == 'near_plane':
        z = 300.0 + 200.0 * torch.rand(H, W, generator=g0)
        z[20:60] = 0.5 + 39.5 * torch.rand(40, W, generator=g0)
    pts = torch.stack([(xs - W / 2 + 0.5) * z / 512.0, (ys - H / 2 + 0.5) * z / 512.0, z]).reshape(1, 3, -1)
    N = W * H
    img, dep = torch.rand(1, 3, N, generator=g0), torch.rand(1, 1, N, generator=g0) * 500 + 100
    # near_depth is a HINT (how many frames share a list: kbe_fused.hip share_plan): one that is far too large makes every group of
    # four frames or more share ONE list whatever its cameras' spread -- the frames must not change
    state = K.prepare_cloud(pts.cuda(), img.cuda(), dep.cuda(), W, H, near_depth=1.0e7)
    assert state['fused']
    K._pack(state)
    cams = [(512.0, (0.9 * i - 12.0, 6.0 - 0.5 * i, -4.0 * i)) for i in range(31)]       # one straight path, equal steps
    if kind == 'curved':
        # what a Ken Burns path is (common.py:88-100: shiftX = dU closestDepth(step) / F): a parabola in shift space -- the cameras
        # between a sub-group's first and last stray from the chord (round 4's straight-line test never let such a group share)
        cams = [(512.0, (0.03 * i * i - 0.9 * i + 3.0, 6.0 - 0.04 * i * i, 2.0 * i - 0.2 * i * i)) for i in range(31)]
    sizes = [12, 5, 12, 2]
    groups, at = [], 0
    for n in sizes:
        groups.append(cams[at:at + n])
        at += n
    want = []
    for g in groups:
        buf = torch.zeros(len(g), H, W, 3, dtype=torch.uint8, device='cuda')
        K.render_frame_group_fused(state, g, 120, buf)
        want.append(c(buf))
    for rep in range(2):
        turns, placed = [0] * 12, False
        for i, g in enumerate(groups):
            n = len(g)
            nxt = groups[i + 1] if i + 1 < len(groups) else None
            ok = nxt is not None and bool(K.lib.kbe_render_frame_group_ahead_ok(N, W, H, n, len(nxt)))
            assert ok or nxt is None
            now = turns[:n]
            for k in range(n):
                turns[k] += 1
            buf = torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
            K.render_frame_group_ahead(state, g, 120, buf, turn=now, placed=placed, next_cameras=nxt if ok else None, next_turn=turns[:len(nxt)] if ok else None)
            placed = ok
            d = np.abs(c(buf).astype(np.int32) - want[i].astype(np.int32))
            assert d.max() <= 1 and (d > 0).mean() < 2e-3, '%s, pass %d group %d: max %d, %.2e differ' % (kind, rep, i, d.max(), (d > 0).mean())
    assert all(w.any() for w in want), 'the frames show something'


@pytest.mark.parametrize('group,n_frames,lanes', [('1', 9, '4'), ('2', 7, '2'), ('12', 30, '2'), ('5', 23, '3')])
def test_video_whose_tile_launches_place_ahead_equals_the_video_with_placement_launches(K, monkeypatch, group, n_frames, lanes):
    """kbe_render_video on the fused route: by default a lane's tile launch makes the placements of the lane's next group;
    KBE_AHEAD=0 (KBE_VIDEO_NO_AHEAD) keeps a placement launch per group.  Same frames, left in HBM and delivered (transfer
    groups ramping 1, 2, 4, ...: the groups of a lane change size), cropped and not, twice in a row, and the frames equal
    frames rendered on their own."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', '1')
    monkeypatch.setenv('KBE_LANES', lanes)
    monkeypatch.setenv('KBE_HOST_LANES', lanes)
    monkeypatch.setenv('KBE_FILL_GROUP', group)
    size = (224, 288)
    settings, oc = _scene(size, 17, 'smooth', True)
    settings = dict(settings, dblSteps=[i / max(n_frames - 1, 1) for i in range(n_frames)])
    cams = common.frame_cameras(settings, oc)
    crop = common.crop_size(settings)
    state = common._prepared_cloud(K, oc)
    assert state['fused']

    def same(a, b, what=''):
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, '%s: max %d, %.2e of the values differ' % (what, d.max(), (d > 0).mean())

    alone = np.stack([K.render_frame(state, sh, f, oc['dblBaseline']).cpu().numpy() for f, sh in cams])
    monkeypatch.setenv('KBE_AHEAD', '0')
    plain = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
    plain_crop = common.render_frames(cams, oc, crop)
    same(plain, alone, 'placement launches, frames left in HBM')
    monkeypatch.delenv('KBE_AHEAD')
    for _ in range(2):
        same(common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy(), plain, 'frames left in HBM')
        same(common.render_frames(cams, oc, None), plain, 'delivered to host memory')
        frames_close(common.render_frames(cams, oc, crop), plain_crop, 'cropped and delivered', cropped=True)
    same(K.render_frame(state, cams[0][1], cams[0][0], oc['dblBaseline']).cpu().numpy(), alone[0], 'a frame on its own after the videos')


def test_delivered_videos_enqueued_back_to_back_without_a_host_synchronisation(K, monkeypatch):
    """kbe_render_video is enqueue-only: a caller may enqueue video after video on one stream and synchronise once.  With the SDMA
    hand-off every call draws signals from the process-wide pool and returns before its copies run; the next call renders into the same
    staging slots.  Thirty videos of different lengths into host buffers of their own, no host synchronisation in between: every frame
    must be the frame of the same video left in HBM (and the pool must hand signals out again afterwards: thirty more)."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', '1')
    size = (160, 224)
    settings, oc = _scene(size, 23, 'smooth', True)
    state = common._prepared_cloud(K, oc)
    lengths = [1, 2, 3, 5, 8, 13, 20, 33, 7, 4]
    videos = []
    for n in lengths:
        cams = common.frame_cameras(dict(settings, dblSteps=[i / max(n - 1, 1) for i in range(n)]), oc)
        want = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
        videos.append((cams, want))
    for _ in range(2):
        hosts = []
        for rep in range(3):
            for cams, want in videos:
                host = torch.zeros(len(cams), size[0], size[1], 3, dtype=torch.uint8, pin_memory=True)
                K.render_video(state, cams, oc['dblBaseline'], None, host_out=host)         # enqueued; no synchronisation
                hosts.append((host, want))
        torch.cuda.current_stream().synchronize()
        for k, (host, want) in enumerate(hosts):
            d = np.abs(host.numpy().astype(np.int32) - want.astype(np.int32))
            assert d.max() <= 1 and (d > 0).mean() < 1e-3, 'video %d of the batch: max %d, %.2e of the values differ' % (k, d.max(), (d > 0).mean())


@pytest.mark.parametrize('n_frames', [20, 1])
def test_a_hand_off_that_fails_behind_an_enqueued_copy_cleans_up_after_itself(K, monkeypatch, n_frames):
    """VERDICT r5 item 4 / ADVICE r5: with the SDMA hand-off a transfer group's copy is enqueued on the engine -- waiting for a release
    signal -- BEFORE the kernel that releases it is launched.  If that launch fails, the copy must neither wait for ever (the engine's
    queue would be wedged for the process) nor fire later into a buffer the caller has freed meanwhile.  KBE_VIDEO_INJECT_FAULT fails the
    second group's hand-off exactly there (the only group's, for a one-frame video).  The call must return KBE_E_LAUNCH, and when it
    has returned nothing may write into its host buffer any more (a pattern written over it stays, the guard frames around it were
    never touched); the next videos of the process -- on the engine again -- are delivered intact; the status call stays clean."""
    from ken_burns_effect_amd import _native, common
    if not _native.handoff_by_sdma():
        pytest.skip('the hand-off under test is the SDMA one')
    monkeypatch.setenv('KBE_FUSED', '1')
    size = (160, 224)
    settings, oc = _scene(size, 29, 'smooth', True)
    state = common._prepared_cloud(K, oc)
    cams = common.frame_cameras(dict(settings, dblSteps=[i / max(n_frames - 1, 1) for i in range(n_frames)]), oc)
    want = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
    guard = 2
    whole = torch.full((n_frames + 2 * guard, size[0], size[1], 3), 0xA5, dtype=torch.uint8).pin_memory()
    host = whole[guard:guard + n_frames]
    monkeypatch.setenv('KBE_INJECT_HANDOFF_FAULT', '1')
    with pytest.raises(_native.KbeError, match='injected hand-off fault'):
        K.render_video(state, cams, oc['dblBaseline'], None, host_out=host)
    monkeypatch.delenv('KBE_INJECT_HANDOFF_FAULT')
    # the call has returned: its copies are over.  Whatever arrives from here on would be a stale copy.
    whole[guard:guard + n_frames] = 0x3C
    torch.cuda.synchronize()
    import time
    time.sleep(0.3)
    assert bool((whole[:guard] == 0xA5).all()) and bool((whole[guard + n_frames:] == 0xA5).all()), 'the guard frames around the buffer'
    assert bool((host == 0x3C).all()), 'a copy of the failed call fired after the call had returned'
    K.handoff_status()                                  # nothing gave up: the engine stays in use
    # the next videos of the process: delivered intact, through the engine (three of them: the signals go round the pool)
    for rep in range(3):
        got = common.render_frames(cams, oc, None)
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, 'video %d after the failed one: max %d, %.2e of the values differ' % (rep, d.max(), (d > 0).mean())


_GIVE_UP_SCRIPT = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
from ken_burns_effect_amd import _native, common
from test_hip_parity import _scene
K = _native.kernels()
os.environ['KBE_FUSED'] = '1'
size = (160, 224)
settings, oc = _scene(size, 31, 'smooth', True)
state = common._prepared_cloud(K, oc)
cams = common.frame_cameras(dict(settings, dblSteps=[i / 39.0 for i in range(40)]), oc)
want = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
K.handoff_status()                                                  # clean so far
host = torch.zeros(len(cams), size[0], size[1], 3, dtype=torch.uint8).pin_memory()
os.environ['KBE_INJECT_HANDOFF_TIMEOUT'] = '1'
K.render_video(state, cams, oc['dblBaseline'], None, host_out=host)
del os.environ['KBE_INJECT_HANDOFF_TIMEOUT']
torch.cuda.current_stream().synchronize()                           # the stream runs on: nothing trapped, the process lives
try:
    K.handoff_status()
    print('NOT-REPORTED')
except _native.KbeError as e:
    print('REPORTED' if 'gave up' in str(e) else 'OTHER: %s' % e)
# the status call waited on the host for the copies that were still under way: the frames are all there now
d = np.abs(host.numpy().astype(np.int32) - want.astype(np.int32))
print('FRAMES-COMPLETE' if d.max() <= 1 and (d > 0).mean() < 1e-3 else 'FRAMES-MISSING max %d' % d.max())
K.handoff_status()                                                  # reported once
print('REPORTED-ONCE')
for rep in range(2):                                                # the engine is off now: the runtime's transfers, same frames
    got = common.render_frames(cams, oc, None)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
print('LATER-VIDEOS-INTACT')
"""


def test_a_hand_off_whose_engine_stops_answering_is_reported_once_and_nothing_traps(tmp_path):
    """the kernel that waits for a transfer group to have left used to trap after 4 s, which the runtime answers by
    aborting the process.  Now it stores into a host-visible error word and returns.  KBE_VIDEO_INJECT_TIMEOUT gives the kernels that wait
    for the lanes' last groups one tick of patience: the stream runs to its end, kbe_video_handoff_status() reports KBE_E_LAUNCH -- once --
    after waiting on the host for the copies still under way (the frames are then complete), and the videos after it, which leave through
    hipMemcpyAsync because the engine stays off, are intact.  In a process of its own: the engine is off for good in a process that saw this."""
    import subprocess
    import sys
    from ken_burns_effect_amd import _native
    if not _native.handoff_by_sdma():
        pytest.skip('the hand-off under test is the SDMA one')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'give_up.py'
    script.write_text(_GIVE_UP_SCRIPT)
    r = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.isupper() or l.startswith(('OTHER', 'FRAMES'))]
    assert lines == ['REPORTED', 'FRAMES-COMPLETE', 'REPORTED-ONCE', 'LATER-VIDEOS-INTACT'], r.stdout[-2000:]


def test_scratch_budget_falls_back_to_fewer_frames_per_launch_and_hint_replaces_the_probe(K, monkeypatch):
    """ADVICE r3 / VERDICT r3 item 6.  (1) The video loop's scratch sets (frames per launch x lanes of them) are capped by a memory
    budget: with KBE_SCRATCH_BUDGET_MB too small for the default shape the loop takes fewer frames per launch -- same frames.
    (2) The lanes of a delivered video measured on rank 0 and handed over with the cloud (`_kbeDeliveryLanes`, sharding.py) are
    taken as they are: no timing probe runs on the rank that received them."""
    from ken_burns_effect_amd import _native, common
    monkeypatch.setenv('KBE_FUSED', '1')
    monkeypatch.setattr(_native, 'PROBE_MIN_FRAMES', 24)         # (the probe runs for videos from 128 frames on; this one has 40)
    size = (224, 288)
    settings, oc = _scene(size, 19, 'smooth', True)
    settings = dict(settings, dblSteps=[i / 39.0 for i in range(40)])
    cams = common.frame_cameras(settings, oc)
    state = common._prepared_cloud(K, oc)
    want = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
    full_sets = state['video_sets']
    assert full_sets == 32                                  # eight frames per scatter launch on four lanes (a zoom-out that fills with the tables)
    stride = int(K.lib.kbe_video_scratch_stride(size[1], size[0], state['N']))
    monkeypatch.setenv('KBE_SCRATCH_BUDGET_MB', str(9 * stride / 1e6))            # room for nine sets: two frames per launch
    got = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
    assert state['video_sets'] == 8
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    monkeypatch.setenv('KBE_SCRATCH_BUDGET_MB', '1')        # less than one set: one frame per launch, one set per lane
    got = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
    assert state['video_sets'] == 4
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    monkeypatch.delenv('KBE_SCRATCH_BUDGET_MB')
    # (2)
    state.pop('delivery_lanes', None)
    state.pop('delivery_probe_us', None)
    oc['_kbeDeliveryLanes'] = {K.zooms_out(state, cams): 3}
    state = common._prepared_cloud(K, oc)
    assert K.delivery_lanes(state, cams, oc['dblBaseline'], None) == 3 and 'delivery_probe_us' not in state
    delivered = common.render_frames(cams, oc, None)
    d = np.abs(delivered.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3 and 'delivery_probe_us' not in state
    del oc['_kbeDeliveryLanes']
    state.pop('delivery_lanes_hint')
    K.delivery_lanes(state, cams, oc['dblBaseline'], None)
    assert 'delivery_probe_us' in state                     # a cloud of one's own: measured


@pytest.mark.parametrize('size', [(50, 37), (33, 64)])
def test_frame_hand_off_with_unaligned_frame_sizes(K, size):
    """W*H*3 not a multiple of 16: the frames of a video start at unaligned host addresses (k_deliver's byte path)."""
    from ken_burns_effect_amd import common
    settings, oc = _scene(size, 5)
    cams = common.frame_cameras(settings, oc)
    host = common.render_frames(cams, oc, None)
    dev = common.render_frames(cams, oc, None, keep_on_device=True).cpu().numpy()
    assert host.shape == dev.shape == (len(cams), size[0], size[1], 3)
    d = np.abs(host.astype(np.int32) - dev.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 2e-3           # two renders: the accumulation order may differ in the last bit
    with pytest.raises(Exception):
        common.render_frames(cams, oc, None, host_out=torch.empty(len(cams), size[0], size[1], 3, dtype=torch.uint8))   # not pinned


def test_render_frame_is_repeatable_and_order_independent(K):
    """Chunk order / layout only affects speed: a shuffled cloud renders the same frame."""
    settings, oc = _scene((256, 320), 4)
    from ken_burns_effect_amd import common
    focal, shift3 = common.frame_cameras(settings, oc)[2]
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], 320, 256)
    a = K.render_frame(state, shift3, focal, 120).clone()
    b = K.render_frame(state, shift3, focal, 120).clone()
    assert (a.int() - b.int()).abs().max() <= 1
    perm = torch.randperm(oc['tensorInpaPoints'].shape[2], device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    s2 = K.prepare_cloud(oc['tensorInpaPoints'][:, :, perm], oc['tensorInpaImage'][:, :, perm], oc['tensorInpaDepth'][:, :, perm], 320, 256)
    cc = K.render_frame(s2, shift3, focal, 120)
    assert (a.int() - cc.int()).abs().max() <= 1 and float((a != cc).float().mean()) < 1e-3


def _grown_scene(size, seed, dolly=False, kind='smooth'):
    """A scene whose cloud has an appended tail like process_inpaint's (common.py:69-80): pixels of a displaced view,
    in that view's raster order, only where a mask says so."""
    settings, oc = _scene(size, seed, kind, dolly)
    gen = torch.Generator('cuda').manual_seed(seed)
    H, W = size
    n = H * W
    pick = torch.nonzero(torch.rand(n, device='cuda', generator=gen) < 0.08).view(-1)
    pts = oc['tensorInpaPoints'][:, :, pick].clone()
    pts[:, 2] *= 1.0 + 0.3 * torch.rand(pick.numel(), device='cuda', generator=gen)          # behind the surface they came from
    pts[:, 0] += 25.0
    pts[:, 1] -= 11.0
    oc['tensorInpaPoints'] = torch.cat([oc['tensorInpaPoints'], pts], 2)
    oc['tensorInpaImage'] = torch.cat([oc['tensorInpaImage'], torch.rand(1, 3, pick.numel(), device='cuda', generator=gen)], 2)
    oc['tensorInpaDepth'] = torch.cat([oc['tensorInpaDepth'], pts[:, 2:3]], 2)
    return settings, oc


@pytest.mark.parametrize('size,dolly,kind', [((96, 128), False, 'smooth'), ((200, 312), False, 'noise'), ((256, 256), True, 'smooth'),
                                             ((37, 50), False, 'smooth'), ((512, 512), False, 'smooth')])
def test_fused_scatter_equals_the_bucket_path(K, size, dolly, kind):
    """The one-launch scatter on the packed cloud (a tile pulls its points through the box hierarchy, z-buffer in LDS)
    against round 1's k_project + k_tiles (global z-buffer, bucket records): z-buffers before and after the degrid
    bit for bit, the same holes, frames within the accumulation order."""
    from ken_burns_effect_amd import common
    settings, oc = _grown_scene(size, 13, dolly, kind)
    H, W = size
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], W, H, 512.0)
    for focal, shift3 in common.frame_cameras(dict(settings, dblSteps=[0.0, 0.35, 1.0]), oc):
        outs = []
        for fused in (True, False):
            rf, ex = torch.empty(4, H, W, device='cuda'), torch.empty(H * W, device='cuda')
            zd, zp = torch.empty_like(ex), torch.empty_like(ex)
            f = K.render_frame(state, shift3, focal, 120, render_f32=rf, existing_f32=ex, zee_f32=zd, zee_pre_f32=zp, fused=fused).clone()
            outs.append((c(f), c(rf), c(ex), c(zd), c(zp)))
        a, b = outs
        assert_bits_equal(a[4], b[4], 'z-buffer before the degrid')
        assert_bits_equal(a[3], b[3], 'z-buffer after the degrid')
        assert np.array_equal(a[2] > 0, b[2] > 0), 'same pixels covered'
        assert np.abs(a[2] - b[2]).max() <= 1e-4 * max(1.0, float(b[2].max()))
        d = np.abs(a[0].astype(np.int32) - b[0].astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
        assert psnr(a[1][:3], b[1][:3], 1.0) > 100.0


def test_tiled_frame_equals_generic_stages(K):
    """The tile renderer against the stage-by-stage global-atomic path (two independent HIP implementations)."""
    settings, oc = _scene((300, 420), 6)           # sizes that are not multiples of the tile or of 4
    from ken_burns_effect_amd import common
    focal, shift3 = common.frame_cameras(settings, oc)[1]
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], 420, 300)
    rf = torch.empty(4, 300, 420, device='cuda')
    ex = torch.empty(300 * 420, device='cuda')
    frame = K.render_frame(state, shift3, focal, 120, render_f32=rf, existing_f32=ex)
    pts = K.shift_points(oc['tensorInpaPoints'], shift3)
    data = torch.cat([oc['tensorInpaImage'], oc['tensorInpaDepth']], 1)
    render, existing = K.render_pointcloud(pts, data, 420, 300, focal, 120, tiled=False)
    filled = K.fill_disocclusion(render, render[:, 3:4] * (existing > 0.0).float())
    assert torch.equal(ex.view(300, 420) > 0, existing[0, 0] > 0)
    assert float((rf - filled[0]).abs().max()) < 1e-4 * max(1.0, float(filled.abs().max()))
    f2 = K.frame_u8(filled)
    assert (frame.int() - f2.int()).abs().max() <= 1


def test_degenerate_points_and_incoherent_clouds(K, oracle):
    """Points at / behind the camera, far outside the view, and a cloud in random order."""
    g0 = torch.Generator().manual_seed(3)
    N = 5000
    pts = torch.rand(1, 3, N, generator=g0) * torch.tensor([1600.0, 1200.0, 900.0]).view(1, 3, 1) - torch.tensor([800.0, 600.0, -100.0]).view(1, 3, 1)
    pts[0, 2, :50] = 0.0
    pts[0, 2, 50:100] = -30.0
    pts[0, 2, 100:120] = 0.004
    img, dep = torch.rand(1, 3, N, generator=g0), torch.rand(1, 1, N, generator=g0) * 500 + 100
    W, H = 200, 136
    state = K.prepare_cloud(pts.cuda(), img.cuda(), dep.cuda(), W, H)
    ok = oracle.OracleKernels('jacobi')
    ostate = ok.prepare_cloud(pts, img, dep, W, H)
    for shift3, focal in (([0.0, 0.0, 0.0], 512.0), ([12.5, -7.0, 40.0], 300.0), ([-3.0, 2.0, -99.0], 512.0)):
        ex = torch.empty(W * H, device='cuda')
        zp = torch.empty_like(ex)
        f = c(K.render_frame(state, shift3, focal, 120, existing_f32=ex, zee_pre_f32=zp))
        ref, _, ref_ex = ok.render_frame(ostate, shift3, focal, 120, want_float=True)
        z0, _ = oracle.zsplat(oracle.shift_points(pts, torch.tensor(shift3)), W, H, focal, 120)
        assert_bits_equal(c(zp).reshape(H, W), z0.numpy()[0, 0], 'z-buffer')
        assert np.array_equal(c(ex).reshape(H, W) > 0, ref_ex.numpy()[0, 0] > 0)
        d = np.abs(f.astype(np.int32) - ref.numpy().astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 2e-3


@pytest.mark.parametrize('per_pixel', [4, 16])
def test_pile_up_paths(K, oracle, per_pixel):
    """Many points per pixel: 4/px exceeds the tile's LDS record capacity (several insert+gather rounds),
    16/px overflows the tile's bucket as well (brute-force path that re-derives the tile from the cloud)."""
    g0 = torch.Generator().manual_seed(per_pixel)
    W, H = 96, 64
    N = per_pixel * W * H
    u = torch.rand(N, generator=g0) * (W + 8) - 4 - W / 2 + 0.5
    v = torch.rand(N, generator=g0) * (H + 8) - 4 - H / 2 + 0.5
    z = torch.rand(N, generator=g0) * 400 + 600
    pts = torch.stack([u * z / 512.0, v * z / 512.0, z]).unsqueeze(0)
    img, dep = torch.rand(1, 3, N, generator=g0), z.view(1, 1, N).clone()
    state = K.prepare_cloud(pts.cuda(), img.cuda(), dep.cuda(), W, H)
    ok = oracle.OracleKernels('jacobi')
    ostate = ok.prepare_cloud(pts, img, dep, W, H)
    shift3, focal = [1.5, -0.75, -20.0], 512.0
    ex, zp, zd = (torch.empty(W * H, device='cuda') for _ in range(3))
    rf = torch.empty(4, H, W, device='cuda')
    f = c(K.render_frame(state, shift3, focal, 120, render_f32=rf, existing_f32=ex, zee_f32=zd, zee_pre_f32=zp))
    ref, ref_float, ref_ex = ok.render_frame(ostate, shift3, focal, 120, want_float=True)
    z0, _ = oracle.zsplat(oracle.shift_points(pts, torch.tensor(shift3)), W, H, focal, 120)
    assert_bits_equal(c(zp).reshape(H, W), z0.numpy()[0, 0], 'z-buffer')
    assert_bits_equal(c(zd).reshape(H, W), oracle.degrid(z0, 'jacobi').numpy()[0, 0], 'degridded z-buffer')
    assert np.abs(c(ex).reshape(H, W) - ref_ex.numpy()[0, 0]).max() <= 1e-4 * float(ref_ex.max())
    assert psnr(c(rf)[:3], ref_float.numpy()[0, :3], 1.0) > 90.0
    d = np.abs(f.astype(np.int32) - ref.numpy().astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3
    # the any-channel-count tile renderer through the same pile-up paths (7 channels: a partial last chunk)
    data = torch.cat([img, dep, torch.rand(1, 3, N, generator=g0)], 1)
    spts = oracle.shift_points(pts, torch.tensor(shift3))
    r_t, e_t = K.render_pointcloud(spts.cuda(), data.cuda(), W, H, focal, 120, tiled=True)
    r_o, e_o = oracle.render_pointcloud(spts, data, W, H, focal, 120, 'jacobi')
    assert np.array_equal(c(e_t) > 0, e_o.numpy() > 0)
    assert np.abs(c(e_t) - e_o.numpy()).max() <= 1e-4 * float(e_o.max())
    assert (np.abs(c(r_t) - r_o.numpy()) <= 1e-4 * np.maximum(np.abs(r_o.numpy()), 1.0)).all()


def test_tiled_render_pointcloud_68_channels_equals_the_atomic_path(K):
    """The inpaint set-up's forward warp (68 channels) two ways: tile gather vs global float atomics."""
    settings, oc = _scene((200, 312), 9)
    from ken_burns_effect_amd import common
    focal, shift3 = common.frame_cameras(settings, oc)[2]
    pts = K.shift_points(oc['tensorInpaPoints'], shift3)
    feat = torch.randn(1, 68, pts.shape[-1], device='cuda', generator=torch.Generator('cuda').manual_seed(2))
    r_t, e_t = K.render_pointcloud(pts, feat, 312, 200, focal, 120, tiled=True)
    r_g, e_g = K.render_pointcloud(pts, feat, 312, 200, focal, 120, tiled=False)
    assert torch.equal(e_t > 0, e_g > 0)
    assert float((e_t - e_g).abs().max()) <= 1e-5 * max(1.0, float(e_g.max()))
    assert float((r_t - r_g).abs().max()) <= 1e-4 * max(1.0, float(r_g.abs().max()))
    # and the scratch is left clean: a second call gives the same result
    r_2, e_2 = K.render_pointcloud(pts, feat, 312, 200, focal, 120, tiled=True)
    assert torch.equal(e_2 > 0, e_t > 0) and float((r_2 - r_t).abs().max()) <= 1e-4 * max(1.0, float(r_t.abs().max()))


def test_pipeline_on_gpu_config2_shape(K):
    """BASELINE.json configs[1] in miniature: 256x256 image through Pipeline (seeded weights) on the GPU."""
    from ken_burns_effect_amd import kbe, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    import warnings
    image, _ = synthetic.make_rgbd(256, 256, 9)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, device='cuda:0', steps=5)
    zoom = kbe.windows_for(256, 256, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), False)
    frames = pipe(image, zoom)
    assert len(frames) == 5 and frames[0].shape == (256, 256, 3) and frames[0].dtype == np.uint8
    assert pipe.objectCommon['tensorInpaPoints'].shape[2] > 256 * 256
    assert np.stack(frames).std() > 1.0


def test_empty_and_single_point_clouds(K):
    z, w = K.zsplat(torch.zeros(1, 3, 0, device='cuda'), 8, 6, 512.0, 120, want_winner=True)
    assert int((K.zkeys_decode(z) != 1000000.0).sum()) == 0 and w.numel() == 0
    pts = torch.tensor([[[0.0], [0.0], [600.0]]], device='cuda')
    r, e = K.render_pointcloud(pts, torch.ones(1, 2, 1, device='cuda'), 8, 6, 512.0, 120)
    assert float(e.sum()) == pytest.approx(1.0, abs=1e-6)


@pytest.mark.parametrize('W,H', [(1, 1), (1, 9), (7, 1), (2, 2)])
def test_one_pixel_wide_rasters_take_the_fp64_image_position(K, oracle, W, H):
    """W or H == 1 is the one case where the fp32 form of common.py:467-468 is NOT the fp64 one (kbe_device.h
    project_xy falls back); z-buffer and winners bit-exact through both splat paths."""
    rng = np.random.default_rng(W * 16 + H)
    N = 200
    z = rng.uniform(30.0, 2000.0, (1, N)).astype(np.float32)
    # image-plane offsets down to 1e-12: tiny positions are where the two forms differ
    u = (rng.uniform(-1.5, 1.5, (1, N)) * 10.0 ** rng.uniform(-12, 0, (1, N))).astype(np.float32) * W
    v = (rng.uniform(-1.5, 1.5, (1, N)) * 10.0 ** rng.uniform(-12, 0, (1, N))).astype(np.float32) * H
    pts = torch.from_numpy(np.stack([u * z / 512.0, v * z / 512.0, z], 1).astype(np.float32))
    zk, win = K.zsplat(pts.cuda(), W, H, 512.0, 120, want_winner=True)
    zo, wo = oracle.zsplat(pts, W, H, 512.0, 120, want_winner=True)
    assert_bits_equal(c(K.zkeys_decode(zk)), zo.numpy(), 'z-buffer %dx%d' % (W, H))
    assert np.array_equal(c(win), wo.numpy())
    data = torch.from_numpy(rng.standard_normal((1, 3, N)).astype(np.float32))
    r_t, e_t = K.render_pointcloud(pts.cuda(), data.cuda(), W, H, 512.0, 120, tiled=True)
    r_o, e_o = oracle.render_pointcloud(pts, data, W, H, 512.0, 120, 'jacobi')
    assert np.array_equal(c(e_t) > 0, e_o.numpy() > 0)
    assert (np.abs(c(r_t) - r_o.numpy()) <= 1e-4 * np.maximum(np.abs(r_o.numpy()), 1.0)).all()


def frames_close(a, b, what='', cropped=False):
    """Two renderings of the same frames: the colour sums depend on the order the records reach a tile (last ulp), so a uint8
    value on an integer boundary may flip by one count.  CROPPED frames have been through the fixed-point arithmetic of
    cv2.getRectSubPix + cv2.resize (common.py:256-257) behind that: one count at one value of the raw frame moves a delivered
    value by TWO in rare places (round 4: (166, 468) -> (155, 492) of a 512 x 512 frame cropped to 460 x 460, found by perturbing the
    raw frame value by value), so there a handful of values may differ by two."""
    d = np.abs(np.asarray(a).astype(np.int32) - np.asarray(b).astype(np.int32))
    bound = 2 if cropped else 1
    assert d.max() <= bound and (d > 0).mean() < 1e-3 and (d > 1).mean() < 1e-5, '%s: max %d, %.2e of the values differ, %.2e by more than one' % (what, d.max(), (d > 0).mean(), (d > 1).mean())


def test_invalid_arguments_return_errors_not_crashes(K):
    import ctypes
    assert K.lib.kbe_zsplat(None, 1, 4, 8, 8, ctypes.c_double(512.0), ctypes.c_double(120.0), None, ctypes.c_void_p(8), None, None) == -1
    assert b'kbe_zsplat' in K.lib.kbe_last_error()
    assert K.lib.kbe_spatial_filter(ctypes.c_void_p(8), 1, 4, 4, 7, ctypes.c_void_p(8), None) == -1
    # the frame loop's size limits (include/kbe.h): rasters with a side of 2^24 or more are refused, not mis-indexed
    z16 = ctypes.c_void_p(16)
    rc = K.lib.kbe_render_frame_stages(z16, z16, z16, 1, 1 << 24, 1, ctypes.c_double(512.0), ctypes.c_double(120.0), None, z16, z16,
                                       None, None, None, None, 7, None, 0, 0, None)
    assert rc == -1 and b'kbe_render_frame' in K.lib.kbe_last_error()
    # ... and from 2^23 on already: k_project's z-splat index is a SIGNED 24-bit multiply, which reads such a width as negative and
    # would drop every splat below the first row.  Refused before anything is enqueued (the pointers are dummies), on every entry of the loop.
    for W, H in ((1 << 23, 1), (1, 1 << 23), (1 << 23, 128)):
        rc = K.lib.kbe_render_frame_stages(z16, z16, z16, 1, W, H, ctypes.c_double(512.0), ctypes.c_double(120.0), None, z16, z16,
                                           None, None, None, None, 7, None, 0, 0, None)
        assert rc == -1 and b'kbe_render_frame' in K.lib.kbe_last_error(), (W, H)
        rc = K.lib.kbe_render_frame_fused(z16, 64, ctypes.c_double(512.0), W, H, ctypes.c_double(512.0), ctypes.c_double(120.0), None, z16, z16,
                                          None, None, None, None, 7, None, -1, None)
        assert rc == -1 and b'kbe_render_frame_fused' in K.lib.kbe_last_error(), (W, H)
        rc = K.lib.kbe_render_pointcloud_tiled(z16, z16, 1, 4, W, H, ctypes.c_double(512.0), ctypes.c_double(120.0), None, z16, z16, z16, None)
        assert rc == -1 and b'kbe_render_pointcloud_tiled' in K.lib.kbe_last_error(), (W, H)
    assert K.lib.kbe_frame_scratch_bytes((1 << 23) - 1, 1, 0) > 0                       # (the size query itself sets no limit)
    # the packed cloud's route addresses a point's 16 bytes by a 32-bit byte offset: clouds of more than 2^28 points are refused
    # there (the plain cloud's route takes them: _native.FUSED_MAX_POINTS)
    rc = K.lib.kbe_render_frame_fused(z16, (1 << 28) + 64, ctypes.c_double(512.0), 64, 64, ctypes.c_double(512.0), ctypes.c_double(120.0), None, z16, z16,
                                      None, None, None, None, 7, None, -1, None)
    assert rc == -1 and b'kbe_render_frame_fused' in K.lib.kbe_last_error()


@pytest.mark.gpu
def test_lanes_and_raster_hints_only_change_speed(K, oracle, monkeypatch):
    """The frame loop spreads consecutive frames over KBE_LANES streams with their own scratch, and k_project
    walks the cloud in patches of a hinted raster: neither may change a frame (up to the accumulation order)."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((96, 160), 11)
    settings = dict(settings, dblSteps=[i / 8.0 for i in range(9)])
    cams = common.frame_cameras(settings, oc)
    crop = common.crop_size(settings)
    frames = {}
    for lanes in ('1', '2', '4'):
        monkeypatch.setenv('KBE_LANES', lanes)
        oc.pop('_kbePreparedCloud', None)
        frames[lanes] = common.render_frames(cams, oc, crop)
        assert common._prepared_cloud(K, oc)['lanes'] == int(lanes)
    for hint in ((32, 32 * 96), (64, 64 * 10), None):             # other raster shapes (every point is still visited once)
        oc.pop('_kbePreparedCloud', None)
        oc['_kbeCloudRaster'] = hint
        frames[str(hint)] = common.render_frames(cams, oc, crop)
    oc.pop('_kbeCloudRaster', None)
    ref = frames['1']
    for key, f in frames.items():
        frames_close(ref, f, key, cropped=True)


@pytest.mark.gpu
def test_denser_than_raster_cloud_matches_oracle(K, oracle):
    """BASELINE.json configs[4] in small: a cloud 4x denser than the target raster (several points per pixel,
    sub-pixel positions), tiled renderer against the oracle."""
    from ken_burns_effect_amd import common, synthetic
    H, W, up = 64, 96, 2
    image, disp = synthetic.make_rgbd(H * up, W * up, 3)
    depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
    pts = K.depth_to_points(depth.cuda(), synthetic.FOCAL * up).view(1, 3, -1)
    img, dep = image.cuda().reshape(1, 3, -1), depth.cuda().reshape(1, 1, -1)
    state = K.prepare_cloud(pts, img, dep, W, H, raster=(W * up, W * up * H * up))
    shift3 = (3.0, -2.0, 8.0)
    rf = torch.empty(4, H, W, device='cuda')
    frame = c(K.render_frame(state, shift3, synthetic.FOCAL, synthetic.BASELINE, render_f32=rf))
    ok = oracle.OracleKernels('jacobi')
    ostate = ok.prepare_cloud(pts.cpu(), img.cpu(), dep.cpu(), W, H)
    oframe = ok.render_frame(ostate, shift3, synthetic.FOCAL, synthetic.BASELINE).numpy()
    d = np.abs(frame.astype(np.int32) - oframe.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 2e-3


@pytest.mark.parametrize('size,dolly,kind', [((512, 512), True, 'smooth'), ((200, 312), False, 'noise'), ((1024, 1024), True, 'smooth'),
                                             ((37, 50), True, 'noise'), ((9, 70), False, 'noise'), ((130, 33), True, 'smooth'), ((257, 1031), True, 'smooth')])
def test_hole_fill_schedules_on_the_same_unfilled_frame_are_byte_identical(K, size, dolly, kind):
    """The three hole-fill schedules (one half-wave per hole; one lane per hole with block skips; one lane per hole with the
    distance table of k_hole_dist) run on the SAME un-filled frame: a fill never reads a hole, so it can be repeated on
    copies, and the copies must agree byte for byte -- the search is the reference's (:838-924) in all three."""
    from ken_burns_effect_amd import common
    settings, oc = _scene(size, 5, kind, dolly)
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], size[1], size[0])
    n_holes = 0
    for focal, shift3 in common.frame_cameras(settings, oc):
        unfilled = K.render_frame(state, shift3, focal, oc['dblBaseline'], stages=3, fused=False).clone()
        results = []
        for mode in (16, 8, 8 | 512, 32 | 512):                     # half-wave, lane, lane + distance table, by count + distance table
            buf = unfilled.clone()
            K.render_frame(state, shift3, focal, oc['dblBaseline'], out=buf, stages=4 | mode, fused=False)
            results.append(buf)
        n_holes += int((results[0] != unfilled).any(dim=2).sum())
        for r in results[1:]:
            assert torch.equal(r, results[0])
    assert n_holes > (1000 if size[0] * size[1] > 50000 else 20)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_hole_fill_schedules_agree_between_islands_of_valid_pixels(K, seed):
    """The tables of the distance-table fill (strips of lines per direction, distances between pixels and between 8 x 8
    blocks) on frames whose valid pixels are islands -- discs, bars and single pixels, image borders included -- with empty
    space and other islands between them: rays that pass islands, graze them, leave the image.  Every hole, every schedule:
    byte-identical to the half-wave search, which has no tables."""
    from ken_burns_effect_amd import synthetic
    H, W = 600, 840
    rng = np.random.default_rng(seed)
    image, disp = synthetic.make_rgbd(H, W, seed, 'smooth')
    depth = ((512.0 * 120) / (disp + 1e-7)).cuda()
    yy, xx = np.mgrid[0:H, 0:W]
    keep = np.zeros((H, W), bool)
    for _ in range(14):                                             # discs
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(6, 90)
        keep |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    for _ in range(6):                                              # thin bars, some touching the border
        x0, y0 = int(rng.uniform(0, W - 200)), int(rng.uniform(0, H - 8))
        keep[y0:y0 + int(rng.uniform(1, 6)), x0:x0 + int(rng.uniform(20, 200))] = True
    keep |= rng.random((H, W)) < 0.0005                             # specks
    keep[:, :3] |= rng.random((H, 3)) < 0.3
    idx = torch.from_numpy(np.flatnonzero(keep)).cuda()
    pts = K.depth_to_points(depth, 512.0).view(1, 3, -1)[:, :, idx].contiguous()
    img = image.cuda().reshape(1, 3, -1)[:, :, idx].contiguous()
    dep = depth.reshape(1, 1, -1)[:, :, idx].contiguous()
    state = K.prepare_cloud(pts, img, dep, W, H, 512.0)
    for shift3, focal in (([0.0, 0.0, 0.0], 512.0), ([30.0, -12.0, -60.0], 400.0)):
        unfilled = K.render_frame(state, shift3, focal, 120, stages=3, fused=False).clone()
        results = []
        for mode in (16, 8, 8 | 512):
            buf = unfilled.clone()
            K.render_frame(state, shift3, focal, 120, out=buf, stages=4 | mode, fused=False)
            results.append(buf)
        assert int((results[0] != unfilled).any(dim=2).sum()) > 20000
        for r in results[1:]:
            assert torch.equal(r, results[0])


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_generate_mask_against_reference_vectors(K, tag):
    """kbe_generate_mask against the reference's own generate_mask kernel (serial order): z-buffer bits, owner
    table, per-point mask, and the median-filtered image (tests/golden/generate_mask.npz)."""
    z = load_golden('generate_mask')
    W, H = int(z[tag + '_W']), int(z[tag + '_H'])
    baseline = int(z[tag + '_baseline']) if bool(z[tag + '_baseline_is_int']) else float(z[tag + '_baseline'])
    masks, zee, ids = K.generate_mask_raw(g(z[tag + '_points']), g(z[tag + '_shift']), W, H, float(z[tag + '_focal']), baseline,
                                          want_tables=True)
    assert_bits_equal(c(zee), z[tag + '_zee_fma'], 'z-buffer')
    assert np.array_equal(c(ids), z[tag + '_ids_fma']), 'owner table'
    assert np.array_equal(c(masks), z[tag + '_masks_raw_fma']), 'per-point mask'
    out = K.generate_mask(g(z[tag + '_points']), g(z[tag + '_shift']), W, H, float(z[tag + '_focal']), baseline)
    assert np.array_equal(c(out), z[tag + '_masks_fma']), 'median-5 of the mask image'


@pytest.mark.gpu
def test_generate_mask_matches_oracle_at_size(K, oracle):
    from ken_burns_effect_amd import synthetic
    H, W, B = 192, 256, 2
    pts, shifts = [], []
    for b in range(B):
        _, disp = synthetic.make_rgbd(H, W, 40 + b)
        depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
        pts.append(oracle.depth_to_points(depth, synthetic.FOCAL).view(1, 3, -1))
        shifts.append([4.0 - 9.0 * b, -3.0, 60.0 * b - 20.0])
    pts, shift = torch.cat(pts, 0), torch.tensor(shifts).view(B, 3, 1)
    masks, zee, ids = K.generate_mask_raw(pts.cuda(), shift.cuda(), W, H, synthetic.FOCAL, synthetic.BASELINE, want_tables=True)
    omasks, ozee, oids = oracle.generate_mask_raw(pts, shift, W, H, synthetic.FOCAL, synthetic.BASELINE)
    assert_bits_equal(c(zee), ozee.numpy(), 'z-buffer')
    assert np.array_equal(c(ids), oids.numpy()) and np.array_equal(c(masks), omasks.numpy())
    assert 0.2 < float(masks.mean()) < 1.0        # a real mix of owners and displaced points


@pytest.mark.gpu
@pytest.mark.parametrize('size,dolly,kind', [((256, 320), True, 'smooth'), ((200, 312), False, 'noise'), ((512, 512), True, 'smooth')])
def test_both_hole_fill_schedules_give_identical_frames(K, size, dolly, kind):
    """One lane per hole (frames with very many holes) against one half-wave per hole: same branch-and-bound
    search, so the filled frames are byte-identical given the same un-filled render (stages 1|2 once, then the
    fill alone in either schedule on copies)."""
    from ken_burns_effect_amd import common
    settings, oc = _scene(size, 5, kind, dolly)
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], size[1], size[0])
    n_filled = 0
    for focal, shift3 in common.frame_cameras(settings, oc):
        outs = []
        for mode in (8, 16, 8 | 512):                               # KBE_STAGE_FILL_PER_LANE, _PER_HALFWAVE, _PER_LANE with the distance table
            rf = torch.zeros(4, size[0], size[1], device='cuda')
            frame = K.render_frame(state, shift3, focal, oc['dblBaseline'], render_f32=rf, stages=7 | mode).clone()
            outs.append((c(frame), c(rf)))
        unfilled = torch.zeros(4, size[0], size[1], device='cuda')
        K.render_frame(state, shift3, focal, oc['dblBaseline'], render_f32=unfilled, stages=3)
        K.render_frame(state, shift3, focal, oc['dblBaseline'], stages=4, fill_rect=(1, 1, 0, 0))      # reset the scratch
        # the un-filled renders of the two runs can differ in the last bit (summation order), so compare what the
        # fill decides: the set of pixels whose float render changed and, where the inputs agree, the values
        for a, b in ((outs[0], outs[1]), (outs[0], outs[2])):
            assert np.array_equal(a[0], b[0]) or (np.abs(a[0].astype(np.int32) - b[0].astype(np.int32)).max() <= 1
                                                  and (a[0] != b[0]).mean() < 1e-3)
        n_filled += int((c(unfilled)[3] == 0).sum())
    assert n_filled > 100


@pytest.mark.parametrize('dolly,step', [(False, 1.0), (True, 0.6)])
def test_full_size_frame_against_the_oracle(K, oracle, dolly, step):
    """BASELINE.json's 1024x1024 configuration, one frame of the KBE path and one of the dolly path (tens of
    thousands of holes, both fill schedules in reach), compared with the CPU oracle pixel by pixel."""
    from ken_burns_effect_amd import common
    settings, oc = _scene((1024, 1024), 0, 'smooth', dolly)
    settings = dict(settings, dblSteps=[step])
    cams = common.frame_cameras(settings, oc)
    frame = common.render_frames(cams, oc, None)[0]
    ok = oracle.OracleKernels('jacobi')
    state = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), 1024, 1024)
    focal, shift3 = cams[0]
    ref = ok.render_frame(state, shift3, focal, oc['dblBaseline']).numpy()
    d = np.abs(frame.astype(np.int32) - ref.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    src = (oc['tensorRawImage'][0].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)
    assert abs(psnr(frame, src, 255.0) - psnr(ref, src, 255.0)) < 1e-3


@pytest.mark.parametrize('fused', ['1', '0'])
def test_one_count_differences_do_not_sit_on_tile_or_patch_edges(K, oracle, monkeypatch, fused):
    """The +-1 count the frame tests allow is summation order (which record reaches a pixel's sum first); it must not hide a
    systematic error of the tiling -- a halo pixel read from the wrong side, a record dropped at a tile's last column.  Float
    renders of four 1024^2 frames against the oracle: (a) where a pixel differs at all it differs by rounding (relative 1e-5), never
    by a contribution; (b) the differing pixels are spread over the tile like all pixels: the share on a tile's border ring (the
    32 x 16 tiles' first / last rows and columns: 17.2 % of the pixels) stays within three points of that geometric share; (c) the
    signed mean difference on the ring is zero to 1e-7 (no bias)."""
    from ken_burns_effect_amd import common
    monkeypatch.setenv('KBE_FUSED', fused)
    settings, oc = _scene((1024, 1024), 4, 'smooth', False)
    settings = dict(settings, dblSteps=[0.0, 0.3, 0.7, 1.0])
    state = K.prepare_cloud(oc['tensorInpaPoints'], oc['tensorInpaImage'], oc['tensorInpaDepth'], 1024, 1024, 512.0)
    assert state['fused'] == (fused == '1')
    ok = oracle.OracleKernels('jacobi')
    ostate = ok.prepare_cloud(oc['tensorInpaPoints'].cpu(), oc['tensorInpaImage'].cpu(), oc['tensorInpaDepth'].cpu(), 1024, 1024)
    yy, xx = np.mgrid[0:1024, 0:1024]
    ring = (xx % 32 == 0) | (xx % 32 == 31) | (yy % 16 == 0) | (yy % 16 == 15)
    share = float(ring.mean())
    n_diff = n_ring = 0
    signed = []
    for focal, shift3 in common.frame_cameras(settings, oc):
        rf, ex = torch.empty(4, 1024, 1024, device='cuda'), torch.empty(1024 * 1024, device='cuda')
        K.render_frame(state, shift3, focal, oc['dblBaseline'], render_f32=rf, existing_f32=ex)
        _, ref, ref_ex = ok.render_frame(ostate, shift3, focal, oc['dblBaseline'], want_float=True)
        a, b = c(rf)[:3], ref[0, :3].numpy()
        assert np.array_equal(c(ex).reshape(1024, 1024) > 0, ref_ex[0, 0].numpy() > 0), 'the same pixels are covered'
        d = a - b
        assert np.abs(d).max() <= 1e-5 * max(1.0, float(np.abs(b).max())), 'a difference larger than rounding: %g' % np.abs(d).max()
        differs = (d != 0).any(axis=0)
        n_diff += int(differs.sum())
        n_ring += int((differs & ring).sum())
        signed.append(float(d[:, ring].mean()))
    assert n_diff > 1000, 'the sums do differ in their last bits somewhere (else this test checks nothing): %d' % n_diff
    assert abs(n_ring / n_diff - share) < 0.03, 'differing pixels on the tiles\' border ring: %.3f of them, %.3f of all pixels' % (n_ring / n_diff, share)
    assert abs(np.mean(signed)) < 1e-7


def test_random_small_scenes_against_the_oracle(K, oracle):
    """Fuzz: random image sizes (down to 1 x 1, not multiples of the tile), random clouds (sparser and denser than
    the raster, points behind the camera and far outside the view) and random cameras; z-buffer bits and frames
    against the oracle."""
    rng = np.random.default_rng(int(os.environ.get('KBE_FUZZ_SEED', '2024')))       # other seeds / more cases: one-off soak runs
    ok = oracle.OracleKernels('jacobi')
    for case in range(int(os.environ.get('KBE_FUZZ_CASES', '120'))):
        scale = int(os.environ.get('KBE_FUZZ_SCALE', '1'))
        H, W = int(rng.integers(1, 90 * scale)), int(rng.integers(1, 140 * scale))
        N = int(rng.integers(0, 4 * H * W + 2))
        focal = float(rng.choice([512.0, 409.6, 153.60000000000002, 64.0]))
        z = rng.uniform(20.0, 3000.0, N).astype(np.float32)
        z[rng.random(N) < 0.02] = rng.choice([0.0, -3.0, 0.0005, 0.01], int((rng.random(N) < 0.02).sum() or 1))[0] if N else 0
        u = rng.uniform(-0.7 * W, 0.7 * W, N).astype(np.float32)
        v = rng.uniform(-0.7 * H, 0.7 * H, N).astype(np.float32)
        pts = torch.from_numpy(np.stack([u * z / np.float32(focal), v * z / np.float32(focal), z])[None].astype(np.float32))
        img = torch.from_numpy(rng.random((1, 3, N), dtype=np.float32))
        dep = torch.from_numpy(np.maximum(z, 1.0)[None, None].astype(np.float32))
        shift3 = [float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5)), float(rng.uniform(-15, 40))]
        state = K.prepare_cloud(pts.cuda(), img.cuda(), dep.cuda(), W, H)
        zp, zd, ex = (torch.empty(W * H, device='cuda') for _ in range(3))
        rf = torch.empty(4, H, W, device='cuda')
        frame = c(K.render_frame(state, shift3, focal, 120, render_f32=rf, existing_f32=ex, zee_f32=zd, zee_pre_f32=zp))
        ostate = ok.prepare_cloud(pts, img, dep, W, H)
        ref, ref_float, ref_ex = ok.render_frame(ostate, shift3, focal, 120, want_float=True)
        z0, _ = oracle.zsplat(oracle.shift_points(pts, torch.tensor(shift3)), W, H, focal, 120)
        tag = 'case %d: %dx%d, %d points, focal %g' % (case, W, H, N, focal)
        assert_bits_equal(c(zp).reshape(H, W), z0.numpy()[0, 0], 'z-buffer, ' + tag)
        assert_bits_equal(c(zd).reshape(H, W), oracle.degrid(z0, 'jacobi').numpy()[0, 0], 'degridded z-buffer, ' + tag)
        # asking for the pre-degrid buffer selects the generic degrid; without it a tile whose z all lie in the
        # band takes the fp32-only, division-free one: same bits
        zd2 = torch.empty(W * H, device='cuda')
        frame_fast = c(K.render_frame(state, shift3, focal, 120, zee_f32=zd2))
        assert_bits_equal(c(zd2).reshape(H, W), c(zd).reshape(H, W), 'degridded z-buffer, fast path, ' + tag)
        assert np.abs(frame_fast.astype(np.int32) - frame.astype(np.int32)).max() <= 1, tag     # (list order = summation order varies)
        assert np.array_equal(c(ex).reshape(H, W) > 0, ref_ex.numpy()[0, 0] > 0), tag
        d = np.abs(frame.astype(np.int32) - ref.numpy().astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 5e-3, tag
        # both hole-fill schedules (sparse clouds leave many holes)
        for mode in (8, 16):
            f2 = c(K.render_frame(state, shift3, focal, 120, stages=7 | mode))
            d2 = np.abs(f2.astype(np.int32) - ref.numpy().astype(np.int32))
            assert d2.max() <= 1 and (d2 > 0).mean() < 5e-3, tag + ', fill schedule %d' % mode


def test_random_render_pointcloud_and_generate_mask_against_the_oracle(K, oracle):
    """Fuzz of the two other users of the splat core: render_pointcloud for random batch / channel counts through the
    tile renderer, and generate_mask on random rasters."""
    rng = np.random.default_rng(7)
    for case in range(40):
        H, W, B, C = int(rng.integers(1, 70)), int(rng.integers(1, 100)), int(rng.integers(1, 3)), int(rng.integers(1, 10))
        N = int(rng.integers(1, 3 * H * W + 2))
        z = rng.uniform(30.0, 2000.0, (B, N)).astype(np.float32)
        u = rng.uniform(-0.6 * W, 0.6 * W, (B, N)).astype(np.float32)
        v = rng.uniform(-0.6 * H, 0.6 * H, (B, N)).astype(np.float32)
        pts = torch.from_numpy(np.stack([u * z / 512.0, v * z / 512.0, z], 1).astype(np.float32))
        data = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32))
        r_t, e_t = K.render_pointcloud(pts.cuda(), data.cuda(), W, H, 512.0, 120, tiled=True)
        r_o, e_o = oracle.render_pointcloud(pts, data, W, H, 512.0, 120, 'jacobi')
        tag = 'case %d: %dx%d B%d C%d N%d' % (case, W, H, B, C, N)
        assert np.array_equal(c(e_t) > 0, e_o.numpy() > 0), tag
        assert (np.abs(c(r_t) - r_o.numpy()) <= 1e-4 * np.maximum(np.abs(r_o.numpy()), 1.0)).all(), tag
    for case in range(30):
        H, W, B = int(rng.integers(3, 60)), int(rng.integers(3, 90)), int(rng.integers(1, 3))     # median-5 reflect-pads by 2
        disp = torch.from_numpy(rng.uniform(10.0, 120.0, (B, 1, H, W)).astype(np.float32))
        depth = (512.0 * 120.0) / (disp + 1e-7)
        pts = oracle.depth_to_points(depth, 512.0).view(B, 3, -1)
        shift = torch.from_numpy(rng.uniform(-20.0, 20.0, (B, 3, 1)).astype(np.float32))
        m, zee, ids = K.generate_mask_raw(pts.cuda(), shift.cuda(), W, H, 512.0, 120, want_tables=True)
        mo, zo, io = oracle.generate_mask_raw(pts, shift, W, H, 512.0, 120)
        assert_bits_equal(c(zee), zo.numpy(), 'generate_mask z-buffer, case %d' % case)
        assert np.array_equal(c(ids), io.numpy()) and np.array_equal(c(m), mo.numpy()), case
        assert np.array_equal(c(K.generate_mask(pts.cuda(), shift.cuda(), W, H, 512.0, 120)), oracle.generate_mask(pts, shift, W, H, 512.0, 120).numpy())


def test_random_crops_against_the_written_algorithm(K, oracle):
    rng = np.random.default_rng(99)
    for case in range(80):
        H, W = int(rng.integers(1, 150)), int(rng.integers(1, 300))
        cw, ch = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out = c(K.crop_resize_u8(torch.from_numpy(f).cuda(), cw, ch))
        assert np.array_equal(out, oracle.crop_resize_u8(f, cw, ch)), 'case %d: %dx%d crop %dx%d' % (case, W, H, cw, ch)


def test_reduced_precision_inpaint_is_opt_in_and_close(K):
    """the GridNet may run in fp16 / bf16 under autocast when asked to; fp32 (the reference's arithmetic)
    is the default and the only setting the parity tests cover."""
    from ken_burns_effect_amd import synthetic
    from ken_burns_effect_amd.pointcloud_inpainting import Inpaint
    net = synthetic.seeded_fill_(Inpaint(), 3).cuda().eval()
    assert net.compute_dtype is None
    g0 = torch.Generator('cuda').manual_seed(5)
    data = torch.randn(1, 68, 96, 128, device='cuda', generator=g0)
    mask = (torch.rand(1, 1, 96, 128, device='cuda', generator=g0) > 0.2).float()
    with torch.no_grad():
        net.normalize_images_disp(torch.rand(1, 3, 96, 128, device='cuda'), torch.rand(1, 1, 96, 128, device='cuda') * 50, not_normed=True)
        base = net.forward(tensorData=data, tensorMasks=mask)
        net.compute_dtype = torch.float16
        half = net.forward(tensorData=data, tensorMasks=mask)
    assert half['tensorImage'].dtype == torch.float32 and half['tensorDisparity'].dtype == torch.float32
    assert float((half['tensorImage'] - base['tensorImage']).abs().max()) < 0.05
    assert float((half['tensorDisparity'] - base['tensorDisparity']).abs().max()) < 0.05 * max(1.0, float(base['tensorDisparity'].abs().max()))


def test_sharded_video_on_the_hip_path_two_ranks():
    """sharding.process_kenburns_sharded with two processes on this GPU (gloo rendezvous on 127.0.0.1): cloud
    broadcast, round-robin frames, gather -- the union equals a single-process render."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                          '--master-port', '29533', os.path.join(root, 'tools', 'sharded_check.py')],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0'))
    assert out.returncode == 0 and 'OK' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_hand_off_turns_with_four_processes_on_one_gpu():
    """Four ranks share this GPU (gloo), each delivering videos to its own pinned host memory on two lanes that take turns on
    the link: every pass delivers the same frames, a rank's second-slowest pass stays within 2.5 times the median pass of all ranks
    and its slowest within 8 times -- the turns' bounded device-side wait is never what a pass waits for in steady state
    (tools/turn_check.py: the bound and what it was measured on)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (no second try: the bound tools/turn_check.py applies allows a rank ONE pass in which the time-sliced ranks stall)
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '4', '--master-addr', '127.0.0.1',
                          '--master-port', '29537', os.path.join(root, 'tools', 'turn_check.py')],
                         capture_output=True, text=True, timeout=900, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0'))
    assert out.returncode == 0 and 'OK' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_scale_report_dry_run_on_one_gpu(tmp_path):
    """tools/scale_report.py --dry-run: the one command that will measure the scaling curve on a node, run here the
    only way a 1-GPU box can -- N = 1 and N = 2 with the two ranks sharing the GPU and the collectives on gloo.  Every path runs (launcher,
    broadcast, weak and strong sharding, per-rank accounts with the NUMA node or the reason there is none); the lines of N = 2 say
    `scaling_valid: false` and the report REFUSES to print a curve from them."""
    import json
    import subprocess
    import sys
    out = str(tmp_path / 'scale.json')
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'KBE_DIST_BACKEND'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'scale_report.py'), '--gpus', '1,2', '--dry-run', '--steps', '12', '--warmup', '4',
                        '--video-frames', '16', '--size', '256', '--out', out], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'weak scaling: NO CURVE' in r.stdout and 'strong scaling: NO CURVE' in r.stdout and 'scaling_valid false' in r.stdout
    doc = json.load(open(out))
    assert doc['dry_run'] and doc['weak_curve'] is None and doc['strong_curve'] is None
    rows = {(x['mode'], x['n_gpus']): x for x in doc['rows']}
    assert set(rows) == {('weak', 1), ('weak', 2), ('strong', 1), ('strong', 2)} and all('error' not in x for x in rows.values())
    for mode in ('weak', 'strong'):
        two = rows[(mode, 2)]
        assert two['ranks_seen'] == 2 and two['collectives'].startswith('gloo') and two['scaling_valid'] is False and two['value'] > 0
        assert two['cloud_broadcast_ms'] is not None and [x['rank'] for x in two['ranks']] == [0, 1]
        assert all(x['numa'] and x['frames'] > 0 and x['ms_per_pass'] > 0 and x['pcie_GBs'] > 0 for x in two['ranks'])
        assert rows[(mode, 1)]['scaling_valid'] is True
    assert sum(x['frames'] for x in rows[('strong', 2)]['ranks']) == 16 and [x['frames'] for x in rows[('weak', 2)]['ranks']] == [12, 12]


def test_numa_binding_of_a_rank_is_best_effort():
    """sharding.bind_to_gpu_numa_node: the CPUs of the GPU's NUMA node, or None (and nothing changed) when unknown."""
    import os
    from ken_burns_effect_amd import sharding
    before = os.sched_getaffinity(0)
    try:
        node = sharding.bind_to_gpu_numa_node(0)
        after = os.sched_getaffinity(0)
        assert (node is None and after == before) or (isinstance(node, int) and node >= 0 and after and after <= before)
    finally:
        os.sched_setaffinity(0, before)


def test_sharded_video_over_rccl_when_the_box_has_two_gpus():
    """The same check on backend "nccl" (= RCCL; one GPU per rank, the cloud broadcast device to device): runs wherever
    two GPUs are visible, skipped on a 1-GPU box.  No scaling curve has been measured yet (no multi-GPU node was
    available to the builder); this keeps the RCCL path from rotting until one is."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                          '--master-port', '29534', os.path.join(root, 'tools', 'sharded_check.py')],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', KBE_DIST_BACKEND='nccl'))
    assert out.returncode == 0 and 'OK (nccl' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_rccl_comes_up_and_takes_the_cloud_broadcast_and_the_frame_gather_with_one_rank():
    """What a 1-GPU box can check of the RCCL path: backend "nccl" initialises on the device, and -- with
    KBE_SINGLE_RANK_COLLECTIVES=1, which keeps a group of one rank from returning early -- the float64 header broadcast, the
    [7, N] fp32 payload broadcast (decoded like a receiver decodes it), the uint8 frame gather and the barrier all run on it;
    the frames must equal the single-process render (tools/sharded_check.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
                          '--master-port', '29541', os.path.join(root, 'tools', 'sharded_check.py')],
                         capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', KBE_DIST_BACKEND='nccl', KBE_SINGLE_RANK_COLLECTIVES='1'))
    assert out.returncode == 0 and 'OK (nccl, 1 ranks)' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_partial_conv_inpainting_pipeline_on_gpu(K):
    """BASELINE.json configs[3] in miniature: the partial-convolution Inpaint (fused HIP mask-update epilogue) driving
    the set-up of a KBE video, and a dolly video (no inpainting, common.py:217), both through Pipeline."""
    from ken_burns_effect_amd import kbe, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    import warnings
    image, _ = synthetic.make_rgbd(192, 256, 12)
    zoom = kbe.windows_for(256, 192, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, partial_inpainting=True, device='cuda:0', steps=4)
        frames = pipe(image, zoom)
        assert len(frames) == 4 and frames[0].shape == (192, 256, 3) and frames[0].dtype == np.uint8
        assert pipe.objectCommon['tensorInpaPoints'].shape[2] > 192 * 256          # the partial-conv net appended points
        dolly = Pipeline(model_paths=None, allow_random_weights=True, partial_inpainting=True, dolly=True, device='cuda:0', steps=4)
        zoom_d = kbe.windows_for(256, 192, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), True)
        frames_d = dolly(image, zoom_d)
    assert len(frames_d) == 4 and dolly.objectCommon['tensorInpaPoints'].shape[2] == 192 * 256
    assert np.stack(frames).std() > 1.0 and np.stack(frames_d).std() > 1.0


def test_bench_times_its_kernels_on_a_cloud_that_keeps_its_placement_launch(K):
    """bench.time_kernels on a cloud twelve times denser than the raster: the one-launch scatter is not available there
    (kbe_render_frame_group_ahead_ok = 0: 24 units of placements per wave), and the timing must fall back to the two launches
    instead of raising (round 3: the configs[4] bench line was lost to exactly that); four times denser (configs[4]) the launch's
    dense form takes the placements along since round 4."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    g0 = torch.Generator().manual_seed(4)
    W, H = 96, 64
    N = 12 * W * H
    u = torch.rand(N, generator=g0) * W - W / 2 + 0.5
    v = torch.rand(N, generator=g0) * H - H / 2 + 0.5
    z = torch.rand(N, generator=g0) * 400 + 600
    pts = torch.stack([u * z / 512.0, v * z / 512.0, z]).unsqueeze(0).cuda()
    oc = {'intWidth': W, 'intHeight': H, 'dblFocal': 512.0, 'dblBaseline': 120.0, 'tensorInpaPoints': pts,
          'tensorInpaImage': torch.rand(1, 3, N, generator=g0).cuda(), 'tensorInpaDepth': z.view(1, 1, N).cuda()}
    assert K.lib.kbe_render_frame_group_ahead_ok(N, W, H, 4, 4) == 0 and K.lib.kbe_render_frame_group_ahead_ok(4 * W * H, W, H, 4, 4) == 1
    kt = bench.time_kernels(oc, [(512.0, (0.5, -0.25, -3.0))] * 3, 'fused', reps=2, group_frames=4)
    assert 'fused:scatter_group' in kt and 'fused:scatter_group_ahead' not in kt and all(v > 0 for v in kt.values() if not isinstance(v, list))
    dense = dict(oc, tensorInpaPoints=pts[:, :, :4 * W * H].contiguous(), tensorInpaImage=oc['tensorInpaImage'][:, :, :4 * W * H].contiguous(),
                 tensorInpaDepth=oc['tensorInpaDepth'][:, :, :4 * W * H].contiguous())
    kt = bench.time_kernels(dense, [(512.0, (0.5, -0.25, -3.0))] * 3, 'fused', reps=2, group_frames=4)
    assert 'fused:scatter_group_ahead' in kt and len(kt['fused:scatter_group_ahead:rounds']) == 5
    sparse = dict(oc, tensorInpaPoints=pts[:, :, :W * H].contiguous(), tensorInpaImage=oc['tensorInpaImage'][:, :, :W * H].contiguous(),
                  tensorInpaDepth=oc['tensorInpaDepth'][:, :, :W * H].contiguous())
    kt = bench.time_kernels(sparse, [(512.0, (0.5, -0.25, -3.0))] * 3, 'fused', reps=2, group_frames=4)
    assert 'fused:scatter_group_ahead' in kt and 'fused:scatter_ahead' in kt
