"""The bar of tests/interval_cases.py held against the CPU oracle alone, so that tests/test_hip_intervals.py can neither be vacuous nor
ask for more than the reference itself delivers: the fp32 oracle in four point orders lies inside every interval and every legal byte
set; on flat 8-bit patches two of those orders differ in more than 1 % of their bytes (why the frames' share bar cannot be carried over
to such images); and a mutant that loses small-weight contributions passes every older bar while it leaves the interval."""
import numpy as np
import pytest
import torch

import interval_cases as ic

BL = ic.BASELINE
CAMS = range(len(ic.CAMERAS))


def fp32_oracle(oracle, name, cam, order):
    """(render [4,H,W], existing [H,W]) of the fp32 oracle on the frame's z-buffer with the cloud in `order`."""
    cs, ref = ic.case(oracle, name), ic.exact_frame(oracle, name, cam)
    o = torch.from_numpy(order)
    pts, data = ic.tensor(ref['points'])[:, :, o].contiguous(), ic.data_of(cs)[:, :, o].contiguous()
    r, e = oracle.normalize(oracle.accumulate(pts, data, ic.tensor(ref['z'])[None, None], ic.CAMERAS[cam][0], BL))
    return r.numpy()[0], e.numpy()[0, 0]


@pytest.mark.parametrize('name', ic.NAMES)
def test_the_fp32_oracle_lies_inside_the_intervals_in_four_point_orders(oracle, name):
    """Assertions 1 and 2: values and weight sums at every covered pixel, every frame byte in its legal set."""
    cs = ic.case(oracle, name)
    for cam in CAMS:
        ref = ic.exact_frame(oracle, name, cam)
        worst_v = worst_w = 0.0
        for k, order in enumerate(ic.point_orders(cs.points.shape[2])):
            what = '%s, camera %d, order %d' % (name, cam, k)
            render, existing = fp32_oracle(oracle, name, cam, order)
            rv, rw = ic.check_intervals(render, existing, ref, what)
            worst_v, worst_w = max(worst_v, rv), max(worst_w, rw)
            two = ic.check_bytes(ic.u8_of(render[:3]).transpose(1, 2, 0), ref, what)
            assert (render[:, ~ref['covered']] == 0).all(), what + ': an uncovered pixel is exactly 0'
            if k == 0:
                assert np.array_equal(render, ref['render']) and np.array_equal(existing, ref['existing'])
        print('%s, camera %d: n <= %d, %d holes; the fp32 oracle at %.2f of the tolerance (weights %.2f); %.4f of the bytes have two legal values'
              % (name, cam, ref['n'].max(), (~ref['covered']).sum(), worst_v, worst_w, two))
        assert ref['covered'].sum() >= 0.5 * ref['covered'].size and ref['n'].max() >= 4
        # the bound is neither missed nor loose: the reference uses between a fifth and all of it
        assert 0.2 <= worst_v <= 1.0 and worst_w <= 1.0


def test_the_cases_reach_what_they_are_there_for(oracle):
    flat, pile4, pile16, odd = (ic.case(oracle, n) for n in ('flat8', 'pile4', 'pile16', 'odd8'))
    assert odd.W % 32 and odd.H % 16                             # csrc/kbe_tiles.h: KBE_TILE_W, KBE_TILE_H
    assert pile4.points.shape[2] == 4 * 96 * 64 and pile16.points.shape[2] == 16 * 96 * 64 == 98304
    img = (flat.image.numpy()[0] * np.float32(255.0)).round().astype(int).T
    assert {tuple(p) for p in np.unique(img, axis=0)} == set(ic.PATCHES)
    for cs in (flat, pile4, odd):                                 # every colour is a byte over 255, divided in fp32
        assert np.array_equal(cs.image.numpy(), np.round(cs.image.numpy() * 255.0).astype(np.float32) / np.float32(255.0))
    a, b = ic.case(oracle, 'flat8_shuffled'), flat
    assert not torch.equal(a.points, b.points) and torch.equal(a.points.sort(2).values, b.points.sort(2).values)
    assert np.array_equal(ic.exact_frame(oracle, 'flat8_shuffled', 1)['z'], ic.exact_frame(oracle, 'flat8', 1)['z'])
    # holes that the fill changes (a step aside opens the bump's flank), holes that it cannot (the dolly focal's border)
    for name in ic.FILL_CASES:
        ref = ic.exact_frame(oracle, name, 1)
        changed = (ref['filled'] != ref['render']).any(0)
        print('%s, camera 1: %d holes, %d filled' % (name, (~ref['covered']).sum(), changed.sum()))
        assert changed.sum() >= 8 and not (changed & ref['covered']).any()
    assert (~ic.exact_frame(oracle, 'flat8', 2)['covered']).sum() >= 1000
    assert ic.exact_frame(oracle, 'pile16', 2)['n'].max() >= 16


def test_two_point_orders_of_flat8_differ_in_more_than_one_percent_of_their_bytes(oracle):
    """Assertion 3.  Every covered value of a flat patch sits an ulp or two from k / 255 and to_u8 truncates: the byte is decided by the
    order of the sum, which the reference leaves undefined.  The frames' bar (one count on < 0.1 % of values) would fail the oracle
    against itself here; 8-bit noise, whose values are nowhere near k / 255, gives 0."""
    n = ic.case(oracle, 'flat8').points.shape[2]
    orders = ic.point_orders(n)
    shares = {}
    for name in ('flat8', 'noise8'):
        a, b = (ic.u8_of(fp32_oracle(oracle, name, 1, orders[k])[0][:3]) for k in (0, 2))
        d = np.abs(a.astype(int) - b.astype(int))
        shares[name] = float((d > 0).mean())
        assert d.max() <= 1
    print('camera 1, point order 0 against 2: %.4f of the bytes of flat8 differ, %.4f of noise8' % (shares['flat8'], shares['noise8']))
    assert shares['flat8'] > 0.01 and shares['noise8'] < 0.001


@pytest.mark.parametrize('name', ic.VIDEO_CASES)
def test_no_choice_of_the_fill_hangs_on_the_last_bits_of_the_depth(oracle, name):
    """What (d) of tests/test_hip_intervals.py rests on: the fill compares the depths of a ray's two ends (common.py:904), and a
    video hands out bytes only.  Filled under the exact depth, under the fp32 oracle's and under depths pushed to either end of
    their interval pixel by pixel, the oracle's unfilled bytes become the oracle's frame."""
    for cam in CAMS:
        ref = ic.exact_frame(oracle, name, cam)
        unfilled = ic.u8_of(ref['render'][:3]).transpose(1, 2, 0)
        tol = ic.tolerance(ref['n'])[0]
        depths = [None, ref['render'][3]]
        for seed in (1, 2):
            sign = np.random.default_rng(seed).choice([-1.0, 1.0], ref['n'].shape)
            depths.append((ref['mean64'][3] * (1.0 + sign * tol)).astype(np.float32))
        for d in depths:
            assert np.array_equal(ic.filled_bytes(oracle, unfilled, ref, d), ref['frame']), '%s, camera %d' % (name, cam)
        assert cam != 1 or (ref['frame'] != unfilled).any(2).sum() >= 16


MUTANT = ('noise8', 1, 1e-4)         # case, camera, share of the pixel's weight sum below which a contribution is lost


def test_a_mutant_that_the_older_bars_pass_leaves_the_interval(oracle):
    """Assertion 4.  On noise8, camera 1, losing every contribution below 1e-4 of its pixel's weight sum (chosen on the CPU: at 1e-3
    the frame differs in 0.13 % of its bytes and the float render reaches 88.6 dB only -- the older bars catch that one; at 1e-4,
    0.003 % and 119 dB) meets every older bar of the frame tests -- bytes within one count on fewer than 0.1 % of values, more than
    100 dB on the float render, `existing` and the render within 1e-4 -- and leaves the interval at a dozen pixels or more."""
    name, cam, below = MUTANT
    ref = ic.exact_frame(oracle, name, cam)
    mean64, wsum64 = ic.dropping_mutant(oracle, name, cam, below)
    render, existing = mean64.astype(np.float32), wsum64.astype(np.float32)
    cov = ref['covered']
    d = np.abs(ic.u8_of(render[:3]).astype(int) - ic.u8_of(ref['render'][:3]).astype(int))
    db = ic.psnr(render[:3], ref['render'][:3])
    rel = np.abs(render - ref['render']) / np.maximum(np.abs(ref['render']), 1.0)
    ex = np.abs(existing - ref['existing']).max() / ref['existing'].max()
    tol_v, tol_w = ic.tolerance(ref['n'])
    out_v = (ic.interval_ratio(render, ref['mean64'], tol_v, cov) > 1.0).any(0)
    out_w = ic.interval_ratio(existing, ref['wsum64'], tol_w, cov) > 1.0
    print('%s, camera %d, contributions below %g lost: bytes max %d on %.5f of the values, %.1f dB, render %.2e, existing %.2e of its maximum; '
          '%d pixels leave the interval of a value, %d of the weight sum' % (name, cam, below, d.max(), (d > 0).mean(), db, rel.max(), ex, out_v.sum(), out_w.sum()))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3 and db > 100.0 and rel.max() <= 1e-4 and ex <= 1e-4, 'the older bars pass it'
    assert np.array_equal(existing > 0, cov)
    assert out_v.sum() >= 12 and out_w.sum() >= 12, 'the interval does not'
    with pytest.raises(AssertionError):
        ic.check_intervals(render, existing, ref, 'the mutant')
