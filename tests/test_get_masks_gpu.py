"""utils.get_masks, the training-side entry on the batched kernels, on the HIP kernel set against the same call on the CPU oracle.

It is the one caller that chains laplacian_valid scaled by the WHOLE batch's maximum, depth_to_points(valid=), a shift per sample and the
batched generate_mask or the batched render_pointcloud with 4 or 68 channels -- on points that are (0, 0, 0) wherever the disparity is not
valid.  tests/test_host_logic.py runs its plumbing on the oracle; here every value it returns is held to the oracle's: masks, shifts and
points bit for bit (generate_mask and the median are exact against the oracle one by one, so must their composition be), renders within
the bound of test_render_pointcloud_whole (tests/test_hip_parity.py).
"""
import numpy as np
import pytest
import torch

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SCENES = [(48, 64, 2), (37, 50, 3), (48, 64, 3), (37, 50, 2)]       # (H, W, B)


@pytest.fixture(scope='module')
def K():
    from ken_burns_effect_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return _native.kernels()


def c(t):
    return t.detach().cpu().numpy()


def scene(H, W, B, scale_first=1.0):
    """test_host_logic's scene: a batch of synthetic.make_rgbd images whose disparities jump at the edges of their rectangles, every sample
    with zoom settings of its own.  scale_first: sample 0's disparity times that -- the batch's maximum, which scales every sample's test."""
    from ken_burns_effect_amd import synthetic
    imgs, disps = zip(*[synthetic.make_rgbd(H, W, 7 + b) for b in range(B)])
    image, disp = torch.cat(imgs), torch.cat(disps).clone()
    disp[0] *= scale_first
    depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
    zoom = {'objectFrom': {'dblCenterU': [W / 2.0] * B, 'dblCenterV': [H / 2.0] * B, 'intCropWidth': [W] * B, 'intCropHeight': [H] * B},
            'objectTo': {'dblCenterU': [W / 2.0 + 3 - 2.5 * b for b in range(B)], 'dblCenterV': [H / 2.0 + 1.5 * b for b in range(B)],
                         'intCropWidth': [int(W * (0.8 - 0.07 * b)) for b in range(B)], 'intCropHeight': [int(H * (0.8 - 0.07 * b)) for b in range(B)]}}
    camera = {'focal': synthetic.FOCAL, 'baseline': synthetic.BASELINE}
    context = torch.randn(B, 64, H, W, generator=torch.Generator().manual_seed(H * W + B))
    return image, disp, depth, zoom, camera, context


def on_both(K, oracle, H, W, B, scale_first=1.0, **kwargs):
    """utils.get_masks(...) on the HIP kernels and on the oracle -> (what the first returned, what the second returned)"""
    from ken_burns_effect_amd import common, utils
    image, disp, depth, zoom, camera, context = scene(H, W, B, scale_first)
    with_context = kwargs.pop('with_context', False)
    results = []
    try:
        for kernel_set, put in ((K, lambda t: t.cuda()), (oracle.OracleKernels('jacobi'), lambda t: t)):
            common._kernel_set = kernel_set
            results.append(utils.get_masks(put(image), put(disp), put(depth), zoom, camera, tensorContext=put(context) if with_context else None, **kwargs))
    finally:
        common._kernel_set = None
    return results


def same_shifts_and_points(got_shift, want_shift, got_objects, want_objects, B):
    assert_bits_equal(c(got_shift), c(want_shift), 'shifts')
    assert len({tuple(s) for s in c(want_shift).reshape(B, 3).tolist()}) == B, 'a shift per sample'
    assert len(got_objects) == len(want_objects) == B
    invalid = 0.0
    for got, want in zip(got_objects, want_objects):
        assert_bits_equal(c(got['tensorRawPoints']), c(want['tensorRawPoints']), 'the points of an objectList entry')
        assert got['objectDepthrange'] == want['objectDepthrange'] and got['dblDispmin'] == want['dblDispmin'] and got['dblDispmax'] == want['dblDispmax']
        invalid += float((c(want['tensorRawPoints']) == 0).all(axis=1).mean()) / B
    assert invalid > 0.01, 'points at the origin: %.4f of the pixels are not valid' % invalid
    return invalid


@pytest.mark.parametrize('H,W,B', SCENES)
def test_get_masks_a_from_b_is_the_oracles_byte_for_byte(K, oracle, H, W, B):
    (masks, shift, objects), (masks0, shift0, objects0) = on_both(K, oracle, H, W, B)
    assert masks.shape == (B, 1, H, W) and masks.is_cuda
    invalid = same_shifts_and_points(shift, shift0, objects, objects0, B)
    assert_bits_equal(c(masks), c(masks0), 'disocclusion masks')
    print('get_masks %dx%d B=%d: %.3f of the pixels invalid, %.3f of the masks set' % (H, W, B, invalid, float(masks0.mean())))
    assert set(np.unique(c(masks0)).tolist()) == {0.0, 1.0}


@pytest.mark.parametrize('tiled', ['1', '0'], ids=['tiled', 'atomic'])
@pytest.mark.parametrize('with_context', [False, True], ids=['4ch', '68ch'])
@pytest.mark.parametrize('H,W,B', SCENES)
def test_get_masks_forward_warp_is_the_oracles_within_the_render_bound(K, oracle, monkeypatch, H, W, B, with_context, tiled):
    """AFromB=False with 4 channels and, under a context, 68: the default route renders a sample at a time through the tile machinery,
    KBE_RENDER_TILED=0 the whole batch with float atomics; either within 2e-5 max(|want|, 1) of the oracle, on the same pixels."""
    monkeypatch.setenv('KBE_RENDER_TILED', tiled)
    (render, holes, points, shift, objects), (render0, holes0, points0, shift0, objects0) = on_both(K, oracle, H, W, B, AFromB=False, with_context=with_context)
    C = 68 if with_context else 4
    assert render.shape == render0.shape == (B, C, H, W) and points.shape == (B, 3, H * W)
    same_shifts_and_points(shift, shift0, objects, objects0, B)
    assert_bits_equal(c(points), c(points0), 'points')
    assert_bits_equal(c(holes), c(holes0), 'hole masks')
    assert 0.0 < float(holes0.mean()) < 1.0
    got, want = c(render), c(render0)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    print('get_masks %dx%d B=%d C=%d tiled=%s: renders within %.3g of the oracle (bound 2e-5)' % (H, W, B, C, tiled, err.max()))
    assert (err <= 2e-5).all()
    assert np.array_equal(got != 0, want != 0), 'the same pixels and channels are touched'
    assert np.array_equal((got != 0).any(axis=1, keepdims=True), c(holes0) > 0)


def test_get_masks_validity_is_scaled_by_the_whole_batchs_maximum(K, oracle):
    """Sample 0's disparity times 3 raises the batch's maximum: the other samples' Laplacians shrink under the same threshold and pixels of
    theirs turn valid.  Both kernel sets change them the same way."""
    H, W, B = 48, 64, 3
    (_, _, objects), (_, _, objects0) = on_both(K, oracle, H, W, B)
    (masks, shift, scaled), (masks0, shift0, scaled0) = on_both(K, oracle, H, W, B, scale_first=3.0)
    assert_bits_equal(c(masks), c(masks0), 'disocclusion masks under the scaled sample')
    assert_bits_equal(c(shift), c(shift0), 'shifts under the scaled sample')
    changed = 0
    for b in range(1, B):
        before, after = c(objects0[b]['tensorRawPoints']), c(scaled0[b]['tensorRawPoints'])
        assert_bits_equal(c(objects[b]['tensorRawPoints']), before, 'sample %d' % b)
        assert_bits_equal(c(scaled[b]['tensorRawPoints']), after, 'sample %d under the scaled sample' % b)
        was_invalid, is_invalid = (before == 0).all(axis=1), (after == 0).all(axis=1)
        assert not (is_invalid & ~was_invalid).any()
        changed += int((was_invalid & ~is_invalid).sum())
    assert changed >= 16, 'pixels of the other samples that the larger maximum makes valid: %d' % changed
