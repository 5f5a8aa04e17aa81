"""The four element-wise kernels the networks run between their convolutions (csrc/kbe_hip.hip: kbe_pconv_epilogue, kbe_prelu_mask,
kbe_bias_act, kbe_upsample2x_act) against the references of tests/network_kernel_cases.py, which tests/test_network_kernel_cases.py pins on
the CPU: bit for bit where the contract is bits (the first three: NumPy float32, one IEEE operation at a time; an expected NaN asks for a
NaN), under a bound per element derived from the number format where it is not (fractional masks, the upsampling) -- at one block and one
thread into the second, on odd sizes, with every operand given and left out, with +-0, +-inf, NaN, subnormals and +-FLT_MAX in the inputs,
with every pointer of bias_act off its 16-byte boundary in turn, and at the grid limits the entries state.

Subnormals: the expectation is IEEE, that is NumPy's.  The MI355X was seen to keep them in all three kernels (no flush on input or
output), so no element is held to anything else.
"""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import network_kernel_cases as nk
from conftest import load_golden

pytestmark = pytest.mark.gpu

KBE_E_INVALID = -1


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def g(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def c(t):
    return t.detach().cpu().numpy()


def void(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_error(K):
    return K.lib.kbe_last_error().decode()


# ---------------------------------------------------------------------------------------
# kbe_pconv_epilogue
# ---------------------------------------------------------------------------------------

def pconv(K, cs, x):
    kw = dict(nk.pconv_kwargs(cs))
    if x['slope'] is not None:
        kw['act_slope'] = g(x['slope'])
    if x['residual'] is not None:
        kw['residual'] = g(x['residual'])
    if cs.operands[1]:
        kw['raw_without_bias'] = True
    out, um = K.pconv_epilogue(g(x['raw']), g(x['bias']), g(x['mask']), cs.k, cs.stride, cs.pad, **kw)
    assert out.shape == (cs.B, cs.Cout, cs.Ho, cs.Wo) and um.shape == (cs.B, 1, cs.Ho, cs.Wo)
    return c(out), c(um)


@pytest.mark.parametrize('geometry', nk.GEOMETRIES, ids=lambda v: 'k%d-s%d-p%d' % v)
def test_pconv_epilogue_on_every_mask_form_and_operand_set(K, geometry):
    """Every case of the geometry (17 x 23, 1 x 1, 5 x 300; 16 x 16 and 1 x 257 where they are one block and one thread more): out and um, bit
    for bit.  A one-channel mask of a layer with several input channels gives the bits of the same mask on every channel."""
    n = 0
    for cs in nk.pconv_cases():
        if (cs.k, cs.stride, cs.pad) == geometry:
            out, um = pconv(K, cs, nk.pconv_inputs(cs))
            want, want_um = nk.pconv_expected(cs)
            nk.assert_same_bits(um, want_um, cs.name + ': um')
            nk.assert_same_bits(out, want, cs.name)
            n += 1
    assert n >= 10


def test_pconv_layer_returns_the_goldens_update_masks(K):
    """PartialConv2d(return_mask=True) on the inputs of tests/golden/partial_conv.npz: the expansion of um is NVIDIA's update mask."""
    from ken_burns_effect_amd.partial_conv import PartialConv2d
    z = load_golden('partial_conv')
    for geometry, tag in nk.GOLDEN_GEOMETRIES.items():
        cin, cout, k, s, p = [int(v) for v in z['cfg_' + tag]]
        layer = PartialConv2d(cin, cout, k, s, p, multi_channel=True, return_mask=True).cuda()
        with torch.no_grad():
            layer.weight.copy_(g(z['w_' + tag]))
            layer.bias.copy_(g(z['b_' + tag]))
            out, mask = layer(g(z['x_' + tag]), mask_in=g(z['m_' + tag]))
        assert mask.shape == out.shape
        nk.assert_same_bits(c(mask), z['mask_' + tag], 'update mask ' + tag)
        _, want_um = nk.pconv_reference(np.zeros(out.shape, np.float32), None, z['m_' + tag], k, s, p)
        nk.assert_same_bits(c(layer.update_mask), want_um, 'um ' + tag)


@pytest.mark.parametrize('cs', nk.SPECIAL_PCONV, ids=lambda cs: cs.name.replace(' ', '-'))
def test_pconv_epilogue_with_special_values_in_raw_and_residual(K, cs):
    """+-0, +-inf, NaN, both ends of the subnormals, +-FLT_MAX and a raw equal to its bias (rb - bv = +0) at scattered elements of raw and of the
    residual: the reference's bits there, and on every other element the bits of the call without them -- nothing leaks into a neighbour."""
    x, touched = nk.pconv_special_inputs(cs)
    out, um = pconv(K, cs, x)
    want, want_um = nk.pconv_expected(cs, x)
    nk.assert_same_bits(um, want_um, cs.name + ': um')
    nk.assert_same_bits(out, want, cs.name)
    clean, _ = pconv(K, cs, nk.pconv_inputs(cs))
    assert nk.same_bits(out, clean)[~touched].all(), 'a special value changed an element that holds none'


@pytest.mark.parametrize('cs', nk.FRACTIONAL_PCONV, ids=lambda cs: cs.name.replace(' ', '-'))
def test_pconv_epilogue_with_fractional_masks_within_the_summation_bound(K, cs):
    """Masks uniform in [0, 1] on all Cin channels: the order of the window sum is nobody's contract, so um and out are held to their float64
    values under the recursive-summation bound, (n - 1) 2^-24 on the sum of n = Cin k k taps, carried through the five operations behind it
    (network_kernel_cases.fractional_bounds has the derivation; to first order (2 (n - 1) + 4) 2^-24 |out| without a bias)."""
    out, um = pconv(K, cs, nk.fractional_inputs(cs))
    out64, um64, out_bound, um_bound = nk.fractional_bounds(cs)
    err_um, err = np.abs(um - um64), np.abs(out - out64)
    print('%s: the kernel uses %.3f of the bound on um and %.3f of the bound on out' %
          (cs.name, (err_um / np.maximum(um_bound, 1e-300)).max(), (err / np.maximum(out_bound, 1e-300)).max()))
    assert (err_um <= um_bound).all() and (err <= out_bound).all()


# ---------------------------------------------------------------------------------------
# kbe_prelu_mask
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', nk.SHAPES, ids=str)
def test_prelu_mask_bit_for_bit(K, shape):
    """0/1, fractional and no mask; a slope of 0, of 1, a negative one and 0.25 among slopes that differ by channel; the special values in x,
    a mask of 0 over +-inf (NaN, as torch.mul gives); then once in place."""
    for form in nk.PRELU_MASK_FORMS:
        x = nk.prelu_mask_inputs(shape, form)
        want = nk.prelu_mask_reference(x['x'], x['slope'], x['mask'])
        nk.assert_same_bits(c(K.prelu_mask(g(x['x']), g(x['slope']), g(x['mask']))), want, 'prelu_mask %s %s' % (shape, form))
    x = nk.prelu_mask_inputs(shape, '01')
    buf = g(x['x'])
    assert K.prelu_mask(buf, g(x['slope']), g(x['mask']), out=buf).data_ptr() == buf.data_ptr()
    nk.assert_same_bits(c(buf), nk.prelu_mask_reference(x['x'], x['slope'], x['mask']), 'prelu_mask %s in place' % (shape,))


# ---------------------------------------------------------------------------------------
# kbe_bias_act
# ---------------------------------------------------------------------------------------

def picked(x, use_b, use_s, n_res):
    return (x['bias'] if use_b else None, x['slope'] if use_s else None, x['res1'] if n_res >= 1 else None, x['res2'] if n_res >= 2 else None)


@pytest.mark.parametrize('shape', nk.BIAS_ACT_SHAPES, ids=str)
def test_bias_act_bit_for_bit(K, shape):
    """Every combination of operands; the special values in x, res1 and res2; a bias that overflows x + bias to inf and an x that cancels its
    bias to +0 (-0 behind a negative slope); then in place."""
    x = nk.bias_act_inputs(shape)
    dev = {k: g(v) for k, v in x.items()}
    for use_b, use_s, n_res in nk.BIAS_ACT_OPERANDS:
        got = K.bias_act(dev['x'], *picked(dev, use_b, use_s, n_res))
        nk.assert_same_bits(c(got), nk.bias_act_reference(x['x'], *picked(x, use_b, use_s, n_res)), 'bias_act %s bias=%s slope=%s residuals=%d' % (shape, use_b, use_s, n_res))
    nk.assert_same_bits(c(dev['x']), x['x'], 'the input of an out-of-place call')
    buf = g(x['x'])
    assert K.bias_act(buf, dev['bias'], dev['slope'], dev['res1'], dev['res2'], out=buf).data_ptr() == buf.data_ptr()
    nk.assert_same_bits(c(buf), nk.bias_act_reference(x['x'], x['bias'], x['slope'], x['res1'], x['res2']), 'bias_act %s in place' % (shape,))


@pytest.mark.parametrize('poison', (0x00, 0xFF))
def test_bias_act_with_each_pointer_off_its_16_byte_boundary(K, poison):
    """HW % 4 == 0: x, res1, res2 and out in turn 4, 8 and 12 bytes off a 16-byte boundary, as contiguous views into a larger buffer.  The
    kernel takes float4 by the alignment of all four: each call gives the aligned call's bits, which are the reference's, and writes
    nothing outside its output."""
    shape = nk.ALIGNMENT_SHAPE
    x = nk.bias_act_inputs(shape)
    want = nk.bias_act_reference(x['x'], x['bias'], x['slope'], x['res1'], x['res2'])
    gd = guarded.Guard(poison)
    bias, slope = g(x['bias']), g(x['slope'])

    def held(name, shift):
        t = gd.empty(shape, torch.float32, 'cuda', shift=shift)
        assert t.data_ptr() % 16 == shift
        if name != 'out':
            t.copy_(g(x[name]))
        return t

    for off in ('none', 'x', 'res1', 'res2', 'out'):
        for shift in ((0,) if off == 'none' else (4, 8, 12)):
            t = {name: held(name, shift if name == off else 0) for name in ('x', 'res1', 'res2', 'out')}
            K.bias_act(t['x'], bias, slope, t['res1'], t['res2'], out=t['out'])
            gd.check()
            nk.assert_same_bits(c(t['out']), want, 'bias_act with %s %d bytes off' % (off, shift))
            for name in ('x', 'res1', 'res2'):
                nk.assert_same_bits(c(t[name]), x[name], 'the input %s' % name)
        gd.release()


@pytest.mark.parametrize('shape', nk.ORDER_SHAPES, ids=str)
def test_bias_act_adds_its_residuals_left_to_right(K, shape):
    """(act(x + b) + r1) + r2 on an r1 of 1e8 and values of order 1 to 10: the other order rounds differently on a fifth of the elements
    (test_network_kernel_cases.py asserts a tenth).  The vector path (32 x 32) and the scalar one (7 x 9)."""
    x = nk.order_inputs(shape)
    dev = {k: g(v) for k, v in x.items()}
    for use_s in (False, True):
        got = K.bias_act(dev['x'], dev['bias'], dev['slope'] if use_s else None, dev['res1'], dev['res2'])
        nk.assert_same_bits(c(got), nk.bias_act_reference(x['x'], x['bias'], x['slope'] if use_s else None, x['res1'], x['res2']), 'bias_act %s' % (shape,))


# ---------------------------------------------------------------------------------------
# kbe_upsample2x_act
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', nk.UPSAMPLE_SHAPES, ids=str)
def test_upsample2x_act_within_the_bound_of_each_output_element(K, shape):
    """Against the float64 value of the kernel's own definition, per output element: 5 2^-24 M, M the largest magnitude among its four taps,
    times 1 + |slope| under the PReLU (network_kernel_cases.upsample_bound) -- on magnitudes over twelve decades, where a tolerance from
    the tensor's maximum would let a wrong weight on a small pixel pass.  Plane (0, 0) is a ramp in x plus another in y: every output
    is exactly representable there and must be exact."""
    x = nk.upsample_inputs(shape)
    B, C, H, W = shape
    for slope in (None, x['slope']):
        got = c(K.upsample2x_act(g(x['x']), g(slope)))
        assert got.shape == (B, C, 2 * H, 2 * W)
        out64, M = nk.upsample_reference(x['x'], slope)
        err = np.abs(got.astype(np.float64) - out64)
        print('upsample2x_act %s slope %s: within %.2f x 2^-24 M' % (shape, slope is not None, (err / np.maximum(nk.U * M, 1e-300)).max()))
        assert (err <= nk.upsample_bound(M, slope)).all()
        nk.assert_same_bits(got[0, 0], out64[0, 0].astype(np.float32), 'the ramp of %s' % (shape,))


def test_upsample2x_act_refuses_to_run_in_place(K):
    x = g(nk.upsample_inputs((2, 3, 7, 9))['x'])
    before = c(x)
    rc = K._raw('kbe_upsample2x_act', void(x), void(None), 2, 3, 7, 9, void(x), stream())
    assert rc == KBE_E_INVALID and last_error(K) == 'kbe_upsample2x_act: bad arguments'
    nk.assert_same_bits(c(x), before, 'x after the refusal')


# ---------------------------------------------------------------------------------------
# the grid limits: B C <= 65535, 2 H <= 65535
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', nk.BIAS_ACT_AT_LIMIT, ids=str)
def test_bias_act_at_the_limit_of_its_grid(K, shape):
    x = nk.limit_inputs(shape)
    got = K.bias_act(g(x['x']), g(x['bias']), g(x['slope']), g(x['res1']))
    nk.assert_same_bits(c(got), nk.bias_act_reference(x['x'], x['bias'], x['slope'], x['res1']), 'bias_act %s' % (shape,))


@pytest.mark.parametrize('shape', nk.UPSAMPLE_AT_LIMIT, ids=str)
def test_upsample2x_act_at_the_limits_of_its_grid(K, shape):
    x = nk.limit_inputs(shape)
    got = c(K.upsample2x_act(g(x['x']), g(x['slope'])))
    out64, M = nk.upsample_reference(x['x'], x['slope'])
    assert (np.abs(got.astype(np.float64) - out64) <= nk.upsample_bound(M, x['slope'])).all()


def test_one_above_their_limits_the_entries_refuse_and_write_nothing(K):
    from ken_burns_effect_amd import _native
    for shape in nk.BIAS_ACT_ABOVE:
        B, C, H, W = shape
        x, out = torch.ones(shape, device='cuda'), torch.full(shape, -7.0, device='cuda')
        assert K._raw('kbe_bias_act', void(x), void(None), void(None), void(None), void(None), B, C, H, W, void(out), stream()) == KBE_E_INVALID
        assert last_error(K) == 'kbe_bias_act: bad arguments'
        with pytest.raises(_native.KbeError, match='kbe_bias_act: bad arguments'):
            K.bias_act(x, out=out)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((x == 1.0).all())
        assert not K.fused_layers_take(shape)
    for shape in nk.UPSAMPLE_ABOVE:
        B, C, H, W = shape
        x, out = torch.ones(shape, device='cuda'), torch.full((B, C, 2 * H, 2 * W), -7.0, device='cuda')
        assert K._raw('kbe_upsample2x_act', void(x), void(None), B, C, H, W, void(out), stream()) == KBE_E_INVALID
        assert last_error(K) == 'kbe_upsample2x_act: bad arguments'
        with pytest.raises(_native.KbeError, match='kbe_upsample2x_act: bad arguments'):
            K.upsample2x_act(x)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
        assert not K.fused_layers_take(shape, upsample=True)
    for shape in nk.BIAS_ACT_AT_LIMIT:
        assert K.fused_layers_take(shape)
    for shape in nk.UPSAMPLE_AT_LIMIT:
        assert K.fused_layers_take(shape, upsample=True)
    assert K.fused_layers_take(nk.UPSAMPLE_ABOVE[1])            # (bias_act has no limit on H)


def close_to_stock(got, stock, what):
    """The bar of test_networks_with_their_element_wise_passes_fused_against_the_stock_modules (tests/test_hip_reference.py)."""
    err, scale = float((got - stock).abs().max()), max(1.0, float(stock.abs().max()))
    print('%s: against the stock modules %.3g (scale %.3g)' % (what, err, scale))
    assert got.shape == stock.shape and err <= 1e-5 * scale, what


def test_a_batch_above_the_limit_runs_through_the_blocks_as_through_the_stock_modules(K, monkeypatch):
    """B C = 65536 (B = 256 on the GridNet's 256-channel row): the blocks used to hand the batch to the fused entries, which refuse it, where
    the stock modules they are made of run.  They ask _native's fused_layers_take now and run such a batch as those modules."""
    from ken_burns_effect_amd import partial_inpainting, pointcloud_inpainting, synthetic
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(nk.CALLER_BATCH, generator=gen).cuda()
    extra = torch.randn(nk.CALLER_BATCH[:2] + (4, 4), generator=gen).cuda()
    with torch.no_grad():
        for name, block, args in (('Basic', pointcloud_inpainting.Basic('relu-conv-relu-conv', (256, 256, 256)), (x,)),
                                  ('Upsample', pointcloud_inpainting.Upsample((256, 256, 256)), (x,)),
                                  # (a block that widens a batch the entries take into one they do not: its first activation fused, the rest not)
                                  ('Basic 128 -> 256', pointcloud_inpainting.Basic('relu-conv-relu-conv', (128, 256, 256)), (x[:, :128].contiguous(),)),
                                  ('Upsample + lateral', pointcloud_inpainting.Upsample((256, 256, 256)), (x, extra))):
            block = synthetic.seeded_fill_(block.eval(), 29).cuda()
            monkeypatch.setenv('KBE_FUSED_LAYERS', '1')
            got = block(*args)
            monkeypatch.setenv('KBE_FUSED_LAYERS', '0')
            stock = block(*args)
            monkeypatch.delenv('KBE_FUSED_LAYERS')
            close_to_stock(got, stock, 'pointcloud_inpainting.%s at %s' % (name, nk.CALLER_BATCH))
        # a batch the entries take still goes through them: the same block on a slice of the batch equals the stock modules too
        small = x[:8].contiguous()
        assert pointcloud_inpainting._fused_layers(small) is K and pointcloud_inpainting._fused_layers(x) is None
        block = synthetic.seeded_fill_(partial_inpainting.Upsample((256, 256, 256)).eval(), 31).cuda()
        mask = (torch.rand((nk.CALLER_BATCH[0], 1, 2, 2), generator=gen) > 0.3).float().cuda()
        got, got_mask = block(x, mask)
        was = getattr(partial_inpainting._Pair._call, 'binary_masks', True)
        partial_inpainting._Pair._call.binary_masks = False         # the unfused route (Inpaint.forward's switch for a fractional mask)
        try:
            stock, stock_mask = block(x, mask)
        finally:
            partial_inpainting._Pair._call.binary_masks = was
        close_to_stock(got, stock, 'partial_inpainting.Upsample at %s' % (nk.CALLER_BATCH,))
        assert torch.equal(got_mask, stock_mask)
