"""The references of tests/network_kernel_cases.py held to what pins them already, and the cases shown to cross what they are there for --
on the CPU alone, so that a later change of a seed or a list cannot quietly empty tests/test_network_kernels_gpu.py:

- the pconv_epilogue restatement against oracle.pconv_epilogue (pinned to NVIDIA's module through tests/golden/partial_conv.npz) on every
  geometry, residual and PReLU added in NumPy;
- the prelu_mask and bias_act restatements against torch's CPU float32 operations, one at a time, special values included;
- the float64 upsampling against F.interpolate on doubles;
- the bounds of the fractional masks and of the upsampling against the kernels' arithmetic restated in NumPy float32.
"""
import numpy as np
import pytest
import torch

import network_kernel_cases as nk
from conftest import load_golden

F = torch.nn.functional


def t(a):
    return None if a is None else torch.from_numpy(np.array(a))


# ---------------------------------------------------------------------------------------
# kbe_pconv_epilogue
# ---------------------------------------------------------------------------------------

def test_the_pconv_cases_cover_what_they_are_to_cover():
    cases = nk.pconv_cases()
    assert len({cs.name for cs in cases}) == len(cases)
    geometries = {(cs.k, cs.stride, cs.pad) for cs in cases}
    assert geometries == set(nk.GEOMETRIES) and len(nk.GEOMETRIES) == 10
    for geometry in nk.GEOMETRIES:
        for form in nk.MASK_FORMS:
            assert any((cs.k, cs.stride, cs.pad) == geometry and cs.form == form and cs.operands == nk.FULL for cs in cases), (geometry, form)
    assert len(nk.OPERANDS) == 12
    for operands in nk.OPERANDS:
        assert len({(cs.k, cs.stride, cs.pad) for cs in cases if cs.operands == operands}) >= 2, operands
    assert {cs.B for cs in cases} == {1, 3} and {cs.Cin for cs in cases} == {1, 3, 5} and {cs.Cout for cs in cases} == {1, 4}
    sizes = {(cs.k, cs.stride, cs.pad, cs.H, cs.W) for cs in cases}
    assert (3, 1, 1, 16, 16) in sizes and (1, 1, 0, 1, 257) in sizes
    for geometry in nk.GEOMETRIES:
        assert geometry + (17, 23) in sizes and geometry + (5, 300) in sizes or geometry[0] > 5, geometry
        assert (geometry + (1, 1) in sizes) == (nk.out_size(1, *geometry) >= 1)
    assert (7, 2, 3, 17, 23) in sizes and (7, 2, 3, 5, 300) in sizes
    blocks = {(cs.Ho * cs.Wo + 255) // 256 for cs in cases}
    assert {1, 2} <= blocks and any(cs.Ho * cs.Wo == 256 for cs in cases) and any(cs.Ho * cs.Wo == 257 for cs in cases)
    assert all(cs.Cin > 1 for cs in cases if cs.form == 'one channel')
    # windows wholly in the padding, with a mask and without one: the update mask and the output are 0 there
    for cs in cases:
        if (cs.k, cs.stride, cs.pad) == (3, 1, 3) and (cs.H, cs.W) == (17, 23):
            out, um = nk.pconv_expected(cs)
            plain, _ = nk.pconv_expected(cs, dict(nk.pconv_inputs(cs), residual=None, slope=None))
            assert (um[:, :, 0, 0] == 0).all() and (um[:, :, -1, -1] == 0).all() and (plain[:, :, 0, 0] == 0).all()
            assert (out[:, :, 0, 0] == nk.prelu(nk.pconv_inputs(cs)['residual'], nk.pconv_inputs(cs)['slope'].reshape(1, -1, 1, 1))[:, :, 0, 0]).all()
            assert cs.form == 'zeros' or (um == 1).any()
    # the rectangle of zeros is larger than the kernel: windows without a valid pixel inside the raster
    for cs in cases:
        if cs.form in ('per channel', 'one channel') and (cs.H, cs.W) == (17, 23):
            _, um = nk.pconv_expected(cs)
            inner = um[:, :, 1:-1, 1:-1] if cs.pad > cs.k // 2 else um
            assert (inner == 0).any() and (um == 1).any(), cs.name


@pytest.mark.parametrize('geometry', nk.GEOMETRIES, ids=lambda g: 'k%d-s%d-p%d' % g)
def test_the_pconv_reference_is_the_oracles(oracle, geometry):
    """Bit for bit, on every case of the geometry: the plain call from the oracle, the residual and the PReLU behind it as NumPy operations;
    raw_without_bias as the oracle on raw + bias.  A one-channel mask gives the oracle's bits both as it is and expanded to Cin channels."""
    for cs in nk.pconv_cases():
        if (cs.k, cs.stride, cs.pad) != geometry:
            continue
        x = nk.pconv_inputs(cs)
        raw = x['raw']
        if cs.operands[1]:
            raw = raw + x['bias'].reshape(1, -1, 1, 1)
        o0, u0 = oracle.pconv_epilogue(t(raw), t(x['bias']), t(x['mask']), cs.k, cs.stride, cs.pad, **nk.pconv_kwargs(cs))
        want = o0.numpy()
        if x['residual'] is not None:
            want = want + x['residual']
        if x['slope'] is not None:
            want = nk.prelu(want, x['slope'].reshape(1, -1, 1, 1))
        out, um = nk.pconv_expected(cs)
        nk.assert_same_bits(out, want, cs.name)
        nk.assert_same_bits(um, u0.numpy(), cs.name + ': um')
        if cs.form == 'one channel':
            direct = nk.pconv_reference(x['raw'], x['bias'], x['mask'], cs.k, cs.stride, cs.pad, cs.Cin, (cs.H, cs.W), x['slope'], x['residual'], cs.operands[1])
            nk.assert_same_bits(direct[0], out, cs.name + ': Cin * msum')
            nk.assert_same_bits(direct[1], um, cs.name + ': Cin * msum, um')


def test_the_pconv_reference_on_the_goldens_of_the_nvidia_module(oracle):
    z = load_golden('partial_conv')
    for geometry, tag in nk.GOLDEN_GEOMETRIES.items():
        cin, cout, k, s, p = [int(v) for v in z['cfg_' + tag]]
        assert (k, s, p) == geometry
        raw = F.conv2d(t(z['x_' + tag]) * t(z['m_' + tag]), t(z['w_' + tag]), t(z['b_' + tag]), stride=s, padding=p).numpy()
        out, um = nk.pconv_reference(raw, z['b_' + tag], z['m_' + tag], k, s, p)
        nk.assert_same_bits(np.broadcast_to(um, out.shape), z['mask_' + tag], 'update_mask ' + tag)
        o0, u0 = oracle.pconv_epilogue(t(raw), t(z['b_' + tag]), t(z['m_' + tag]), k, s, p)
        nk.assert_same_bits(out, o0.numpy(), 'the oracle on golden ' + tag)
        nk.assert_same_bits(um, u0.numpy(), 'the oracle on golden %s: um' % tag)


def test_the_pconv_special_values_reach_every_branch():
    for cs in nk.SPECIAL_PCONV:
        x, touched = nk.pconv_special_inputs(cs)
        assert np.isnan(x['raw']).any() and np.isinf(x['raw']).any() and nk.is_subnormal(x['raw']).any() and (np.abs(x['raw']) == nk.FLT_MAX).any()
        assert (x['raw'] == x['bias'].reshape(1, -1, 1, 1)).any() and (x['raw'] == -x['bias'].reshape(1, -1, 1, 1)).any()
        clean, _ = nk.pconv_expected(cs)
        out, _ = nk.pconv_expected(cs, x)
        assert nk.same_bits(out, clean)[~touched].all(), 'the reference itself keeps a special value to its element'
        assert np.isnan(out[touched]).any() and 0.01 < touched.mean() < 0.5
    assert {cs.form for cs in nk.SPECIAL_PCONV} == {'per channel', 'none'} and len(nk.SPECIAL_PCONV) == 8


@pytest.mark.parametrize('cs', nk.FRACTIONAL_PCONV, ids=lambda cs: cs.name.replace(' ', '-'))
def test_the_fractional_bound_holds_for_the_kernels_loop_order(cs):
    """The float32 restatement in the kernel's order (channel, ky, kx) stays within the derived bound of the float64 value."""
    x = nk.fractional_inputs(cs)
    out64, um64, out_bound, um_bound = nk.fractional_bounds(cs)
    out, um = nk.pconv_reference(x['raw'], x['bias'], x['mask'], cs.k, cs.stride, cs.pad, cs.Cin, (cs.H, cs.W))
    worst_um = float((np.abs(um - um64) / np.maximum(um_bound, 1e-300)).max())
    worst = float((np.abs(out - out64) / np.maximum(out_bound, 1e-300)).max())
    print('%s: the float32 restatement uses %.3f of the bound on um, %.3f of the bound on out' % (cs.name, worst_um, worst))
    assert (np.abs(um - um64) <= um_bound).all() and (np.abs(out - out64) <= out_bound).all()
    assert ((um64 > 0) & (um64 < 1)).any() and (um64 == 1).any(), 'sums on both sides of the clamp'
    # ... and sums well inside (1, 2): a clamp that began at 2 would leave um = msum there, a thousand bounds from 1
    msum, _ = nk.window_sums(cs.B, x['mask'], cs.k, cs.stride, cs.pad, dtype=np.float64)
    assert ((msum > 1.05) & (msum < 1.95)).sum() >= 4 and 0.05 > 1000 * um_bound.max()
    n = cs.Cin * cs.k * cs.k
    if x['bias'] is None:
        assert np.allclose(out_bound, (2 * (n - 1) + 4) * nk.U * np.abs(out64), rtol=1e-3), 'the first-order form of the docstring'


# ---------------------------------------------------------------------------------------
# kbe_prelu_mask, kbe_bias_act
# ---------------------------------------------------------------------------------------

def test_the_slopes_differ_by_channel_and_hold_the_four_named_ones():
    seen = set()
    for shape in nk.SHAPES + nk.BIAS_ACT_SHAPES + nk.UPSAMPLE_SHAPES:
        seen |= set(nk.prelu_mask_inputs(shape, 'none')['slope'].tolist()) | set(nk.upsample_inputs(shape)['slope'].tolist())
    assert {0.0, 1.0, -0.5, 0.25} <= seen
    for shape in [(2, 3, 7, 9), (3, 4, 17, 23)]:
        for slope in (nk.prelu_mask_inputs(shape, '01')['slope'], nk.bias_act_inputs(shape)['slope'], nk.upsample_inputs(shape)['slope']):
            assert len(set(slope.tolist())) == shape[1] and (slope < 0).any()


@pytest.mark.parametrize('shape', nk.SHAPES, ids=str)
def test_the_prelu_mask_reference_is_torchs(shape):
    for form in nk.PRELU_MASK_FORMS:
        x = nk.prelu_mask_inputs(shape, form)
        want = F.prelu(t(x['x']), t(x['slope']))
        if x['mask'] is not None:
            want = want * t(x['mask'])
        got = nk.prelu_mask_reference(x['x'], x['slope'], x['mask'])
        nk.assert_same_bits(got, want.numpy(), 'prelu_mask %s %s' % (shape, form))
        if form != 'none' and np.isinf(x['x']).any():
            assert np.isnan(got[np.isinf(x['x'])]).all(), 'a mask of 0 over an infinity is NaN'
    if np.prod(shape) >= len(nk.SPECIALS):
        v = nk.prelu_mask_inputs(shape, 'none')['x']
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and nk.is_subnormal(v).any() and (np.abs(v) == nk.FLT_MAX).any()
        assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()


@pytest.mark.parametrize('shape', nk.BIAS_ACT_SHAPES, ids=str)
def test_the_bias_act_reference_is_torchs(shape):
    x = nk.bias_act_inputs(shape)
    for use_b, use_s, n_res in nk.BIAS_ACT_OPERANDS:
        want = t(x['x'])
        want = want + t(x['bias']).view(1, -1, 1, 1) if use_b else want
        want = F.prelu(want, t(x['slope'])) if use_s else want
        want = want + t(x['res1']) if n_res >= 1 else want
        want = want + t(x['res2']) if n_res >= 2 else want
        got = nk.bias_act_reference(x['x'], x['bias'] if use_b else None, x['slope'] if use_s else None, x['res1'] if n_res >= 1 else None,
                                    x['res2'] if n_res >= 2 else None)
        nk.assert_same_bits(got, want.numpy(), 'bias_act %s %s' % (shape, (use_b, use_s, n_res)))
    summed = nk.bias_act_reference(x['x'], x['bias'])
    assert ((summed == 0) & ~np.signbit(summed)).any(), 'an x that cancels its bias to +0'
    if shape[1] > 1 and shape[2] * shape[3] > 4:
        assert np.isposinf(summed[np.isfinite(x['x'])]).any(), 'a finite x + bias that overflows'
    if (x['slope'] < 0).any() and shape[2] * shape[3] > 1:
        acted = nk.bias_act_reference(x['x'], x['bias'], x['slope'])
        assert ((acted == 0) & np.signbit(acted) & (summed == 0) & ~np.signbit(summed)).any(), 'a negative slope times +0 is -0'


@pytest.mark.parametrize('shape', nk.ORDER_SHAPES, ids=str)
def test_the_reference_tells_the_two_orders_of_the_residuals_apart(shape):
    x = nk.order_inputs(shape)
    for slope in (None, x['slope']):
        a = nk.bias_act_reference(x['x'], x['bias'], slope, x['res1'], x['res2'])
        b = nk.bias_act_reference(x['x'], x['bias'], slope, x['res1'], x['res2'], swap_residuals=True)
        share = float((~nk.same_bits(a, b)).mean())
        print('bias_act %s: the two orders differ on %.3f of the elements' % (shape, share))
        assert share >= 0.1
        nk.assert_same_bits(a, ((F.prelu(t(x['x']) + t(x['bias']).view(1, -1, 1, 1), t(slope)) if slope is not None else t(x['x']) + t(x['bias']).view(1, -1, 1, 1))
                                + t(x['res1']) + t(x['res2'])).numpy(), 'the order of the separate passes')


# ---------------------------------------------------------------------------------------
# kbe_upsample2x_act
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', nk.UPSAMPLE_SHAPES, ids=str)
def test_the_float64_upsampling_is_torchs_and_the_float32_one_within_the_bound(shape):
    x = nk.upsample_inputs(shape)
    for slope in (None, x['slope']):
        out64, M = nk.upsample_reference(x['x'], slope)
        want = F.interpolate(t(x['x']).double(), scale_factor=2, mode='bilinear', align_corners=False)
        if slope is not None:
            want = F.prelu(want, t(slope).double())
        want = want.numpy()
        assert (np.abs(out64 - want) <= 1e-12 * np.abs(want)).all()
        out32, _ = nk.upsample_reference(x['x'], slope, dtype=np.float32)
        units = np.abs(out32.astype(np.float64) - out64) / np.maximum(nk.U * M, 1e-300)
        print('upsample %s slope %s: the float32 restatement is within %.2f u M' % (shape, slope is not None, units.max()))
        assert (np.abs(out32.astype(np.float64) - out64) <= nk.upsample_bound(M, slope)).all()
        # the ramp: every output of plane (0, 0) is exactly representable, and float32 arithmetic finds it
        nk.assert_same_bits(out32[0, 0], out64[0, 0].astype(np.float32), 'the ramp')
        assert (out64[0, 0].astype(np.float32).astype(np.float64) == out64[0, 0]).all()


def test_exchanged_column_weights_leave_the_bound_on_the_ramp_and_on_small_pixels():
    shape = (3, 4, 17, 23)
    x = nk.upsample_inputs(shape)
    out64, M = nk.upsample_reference(x['x'])
    wrong, _ = nk.upsample_reference(x['x'], dtype=np.float32, swap_columns=True)
    off = np.abs(wrong.astype(np.float64) - out64) > nk.upsample_bound(M)
    assert off[0, 0, :, 1:-1].all(), 'every interior column of the ramp'
    # ... and a tolerance taken from the tensor's maximum would not have seen a twentieth of them or more
    hidden = float((np.abs(wrong.astype(np.float64) - out64) <= 4e-7 * np.abs(x['x']).max())[off].mean())
    print('exchanged column weights: %.3f of the outputs leave the bound, %.3f of those within 4e-7 of the maximum' % (off.mean(), hidden))
    assert hidden >= 0.05


def test_the_sizes_put_a_block_boundary_between_two_threads():
    widths = {shape[3] for shape in nk.UPSAMPLE_SHAPES}
    assert {1, 255, 256, 257} <= widths and any(shape[2] == 1 for shape in nk.UPSAMPLE_SHAPES) and any(w % 2 for w in widths)
    assert any(shape[2] * shape[3] == 256 for shape in nk.SHAPES) and any(shape[2] * shape[3] == 257 for shape in nk.SHAPES)
    assert {shape[2] * shape[3] // 4 for shape in nk.BIAS_ACT_SHAPES if shape[2] * shape[3] % 4 == 0} >= {256, 264}
    for shape in nk.BIAS_ACT_AT_LIMIT + nk.UPSAMPLE_AT_LIMIT:
        assert shape[0] * shape[1] == 65535 or 2 * shape[2] + 1 == 65535
    for shape in nk.BIAS_ACT_ABOVE + nk.UPSAMPLE_ABOVE:
        assert shape[0] * shape[1] == 65536 or shape[2] == 32768
    assert nk.CALLER_BATCH[0] * nk.CALLER_BATCH[1] == 65536


def test_the_callers_predicate_draws_the_line_where_the_entries_do():
    """HipKernels.fused_layers_take (what the blocks ask before they hand a tensor to kbe_bias_act / kbe_upsample2x_act) against the limits
    of csrc/kbe_hip.hip's KBE_REQUIRE lines, which the GPU test holds the entries to: B C <= 65535, and 2 H <= 65535 for the upsampling."""
    from ken_burns_effect_amd._native import HipKernels
    take = HipKernels.fused_layers_take
    assert all(take(shape) for shape in nk.BIAS_ACT_AT_LIMIT) and not any(take(shape) for shape in nk.BIAS_ACT_ABOVE)
    assert all(take(shape, upsample=True) for shape in nk.UPSAMPLE_AT_LIMIT) and not any(take(shape, upsample=True) for shape in nk.UPSAMPLE_ABOVE)
    assert take((1, 1, 32768, 1)) and not take(nk.CALLER_BATCH) and take((255, 256, 2, 2), upsample=True)
