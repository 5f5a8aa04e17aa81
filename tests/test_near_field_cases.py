"""The cases of tests/near_field_cases.py cross what they are there for -- shown on the CPU oracle alone, so that a later change of a
seed or a pattern cannot quietly empty tests/test_hip_near_field.py: the fp32-comparison mutants of the degrid and of the z test differ
from the oracle on `edge19` by the margins below; `band_tiles` holds a tile of every class of the per-tile band decision; the z-buffers
hold negative values, the empty key under a weight, and waves that mix the regimes."""
import numpy as np
import pytest
import torch

import near_field_cases as nf
from conftest import assert_bits_equal

F, BL = nf.FOCAL, nf.BASELINE


def frames_of(name):
    return range(len(nf.case(name).cameras))


def test_the_depths_at_the_edge_are_found_not_written_down():
    z, err, down, up = nf.edge19_depths()
    print('edge19: %d consecutive depths %.9g..%.9g reach %d values of dblError; %d pairs c < a + 1, %d pairs c > a + 1'
          % (z.size, z[0], z[-1], np.unique(err).size, len(down), len(up)))
    assert (np.diff(z.view(np.uint32).astype(np.int64)) == 1).all() and z.size > 250
    assert err.min() < nf.BAND_LO < err.max()
    for pairs, sign in ((down, -1), (up, 1)):
        assert len(pairs) >= 2
        for za, zc in pairs:
            a, c = nf.dbl_error(za), nf.dbl_error(zc)
            assert c == np.float32(a + np.float32(1.0)) and np.sign(float(c) - (float(a) + 1.0)) == sign
            assert a < nf.BAND_LO <= c


@pytest.mark.parametrize('name', nf.NAMES)
def test_the_fp64_restatement_of_the_degrid_is_the_oracles(oracle, name):
    for cam in frames_of(name):
        ref = nf.oracle_frame(oracle, name, cam)
        assert_bits_equal(nf.degrid_restated(ref['z_pre'], np.float64), ref['z'], '%s, camera %d' % (name, cam))


def test_the_mutants_differ_from_the_oracle_on_edge19(oracle):
    """An fp32 `c >= a + 1.0f` in the degrid, an fp32 `err <= zee + 1.0f` in the accumulation: what a kernel that took its in-band
    branch outside the band would compute."""
    cs, ref = nf.case('edge19'), nf.oracle_frame(oracle, 'edge19', 0)
    witnesses = nf.edge19_witnesses()
    assert not nf.in_band(ref['z_pre']).all() and nf.in_band(ref['z_pre']).any()
    degrid_diff = nf.degrid_restated(ref['z_pre'], np.float32) != ref['z']
    moved = _fp32_ztest_moves(oracle, 'edge19')
    untouched = witnesses & (ref['z'] == ref['z_pre'])
    print('edge19: the fp32 degrid differs at %d pixels (%d in rows 0..31); the fp32 z test moves `existing` by >= 0.25 at %d pixels, '
          '%d of them the %d witnesses (max %.4f; the tolerance on the GPU is %.1e)'
          % (degrid_diff.sum(), degrid_diff[:32].sum(), (moved >= 0.25).sum(), (moved[untouched] >= 0.25).sum(), witnesses.sum(), moved.max(),
             1e-4 * ref['existing'].max()))
    assert degrid_diff.sum() >= 64 and degrid_diff[:32].sum() >= 64
    assert untouched.sum() == witnesses.sum() >= 16, 'no witness of the z test is degridded'
    assert (moved >= 0.25).sum() >= 16 and (moved[untouched] >= 0.25).sum() >= 16
    assert 0.25 > 1000 * 1e-4 * ref['existing'].max()


def _fp32_ztest_moves(oracle, name, cam=0):
    """|existing of the oracle's accumulation deciding as the fp32 sum zee + 1.0f would - existing|: the z test alone, on the oracle's z-buffer."""
    cs, ref = nf.case(name), nf.oracle_frame(oracle, name, cam)
    zee = nf.tensor(nf.fp32_ztest_zee(ref['z']))[None, None]
    acc = oracle.accumulate(nf.tensor(ref['points']), torch.cat([cs.image, cs.depth], 1), zee, F, BL)
    return np.abs(oracle.normalize(acc)[1].numpy()[0, 0] - ref['existing'])


def test_band_tiles_holds_a_tile_of_every_class(oracle):
    for name in ('band_tiles', 'band_tiles_50x37'):
        cs, ref = nf.case(name), nf.oracle_frame(oracle, name, 0)
        classes = nf.tile_band_classes(ref['z_pre'])
        count = {k: sum(1 for v in classes.values() if v == k) for k in ('band', 'inside', 'edge', 'diagonal')}
        wx, wy = nf.BAND_TILES_WITNESS[(cs.W, cs.H)]
        moved = _fp32_ztest_moves(oracle, name)
        print('%s: tiles by where their out-of-band values are: %s; %d pixels outside the band, all between %.0f and %.0f; the fp32 z test moves '
              '`existing` by %.4f at the witness (%d, %d)' % (name, count, (~nf.in_band(ref['z_pre'])).sum(), ref['z_pre'].min(),
                                                              ref['z_pre'][~nf.in_band(ref['z_pre'])].max(), moved[wy, wx], wx, wy))
        near = np.zeros((cs.H, cs.W), bool)
        for x, y in nf.BAND_TILES_NEAR[(cs.W, cs.H)]:
            near[y, x] = True
        assert np.array_equal(~nf.in_band(ref['z_pre']), near), 'the pixels outside the band are the listed ones'
        assert moved[wy, wx] >= 0.25 and ref['z'][wy, wx] == ref['z_pre'][wy, wx] < 131072.0
        if name == 'band_tiles':
            assert min(count.values()) >= 1
            assert classes[(0, 0)] == 'inside' and classes[(1, 2)] == 'edge' and classes[(1, 0)] == 'edge' and classes[(0, 1)] == 'edge'
            assert classes[(1, 1)] == 'diagonal' and classes[(2, 2)] == 'inside' and classes[(2, 3)] == 'inside' and classes[(2, 0)] == 'band'
        else:
            assert 50 % nf.TILE_W and 37 % nf.TILE_H and classes[(1, 2)] == 'inside' and classes[(1, 1)] == 'inside' and count['band'] >= 1


def _first_index_per_pixel(winner, select, n_pixels):
    first = np.full(n_pixels, np.iinfo(np.int64).max)
    idx = np.flatnonzero(select & (winner >= 0))
    np.minimum.at(first, winner[idx], idx)
    return first


def test_negative_values_win_and_lose_in_either_order(oracle):
    cs = nf.case('negative')
    for cam in frames_of('negative'):
        ref = nf.oracle_frame(oracle, 'negative', cam)
        err = nf.dbl_error(ref['points'][0, 2])
        hw = cs.W * cs.H
        neg = _first_index_per_pixel(ref['winner'], err < 0, hw)
        pos = _first_index_per_pixel(ref['winner'], err > 0, hw)
        none = np.iinfo(np.int64).max
        both = (neg != none) & (pos != none)
        neg_count = np.bincount(ref['winner'][(ref['winner'] >= 0) & (err < 0)], minlength=hw)
        z = ref['z_pre'].reshape(-1)
        print('negative, camera %d: %d pixels won by a negative dblError (min %.4g), on %d it beats a positive one (%d arriving after it, %d before), '
              '%d pixels with two or more negative values, %d holes'
              % (cam, (z < 0).sum(), z.min(), both.sum(), (both & (neg > pos)).sum(), (both & (neg < pos)).sum(), (neg_count >= 2).sum(), (ref['existing'] <= 0).sum()))
        assert (z < 0).sum() >= 16 and (z[both] < 0).all() and both.sum() >= 16
        assert (both & (neg > pos)).sum() >= 16 and (both & (neg < pos)).sum() >= 16
        assert (neg_count >= 2).sum() >= 16
        assert (ref['existing'] <= 0).sum() >= 16, 'holes for the fill'
    z0 = nf.oracle_frame(oracle, 'negative', 0)['z_pre']
    assert z0.min() < -5e7 and ((z0 > -1000) & (z0 < 0)).any() and ((z0 >= 0) & (z0 < nf.BAND_LO)).any()


def test_far_points_keep_the_empty_key_under_a_weight(oracle):
    cs = nf.case('far')
    for cam in frames_of('far'):
        ref = nf.oracle_frame(oracle, 'far', cam)
        err = nf.dbl_error(ref['points'][0, 2])
        far = (err == nf.EMPTY) & (ref['points'][0, 2] >= nf.Z_CULL)
        covered = (ref['z_pre'] == nf.EMPTY) & (ref['existing'] > 0)
        holes = ref['existing'] <= 0
        reached = np.zeros(cs.W * cs.H, bool)
        reached[ref['winner'][far & (ref['winner'] >= 0)]] = True
        loses = reached.reshape(cs.H, cs.W) & (ref['z_pre'] < nf.EMPTY - 1)
        print('far, camera %d: %d points with dblError == 1e6 (%d beyond 1e30); %d pixels with the empty key and a weight, %d holes, '
              '%d pixels where such a point loses' % (cam, far.sum(), (ref['points'][0, 2] >= 1e30).sum(), covered.sum(), holes.sum(), loses.sum()))
        assert covered.sum() >= 16 and holes.sum() >= 16 and loses.sum() >= 16
        assert (ref['points'][0, 2] >= 1e30).sum() >= 8


def test_mixed_mixes_the_regimes_within_64_points(oracle):
    cs = nf.case('mixed')
    n = cs.points.shape[2] // 64 * 64
    for cam in frames_of('mixed'):
        ref = nf.oracle_frame(oracle, 'mixed', cam)
        z = ref['points'][0, 2, :n].reshape(-1, 64)
        live = z >= nf.Z_CULL
        counts = {}
        for what, lo in (('2', 2.0), ('16', 16.0)):
            counts[what] = int((((z < lo) & live).any(1) & (z >= lo).any(1)).sum())
        counts['1e30'] = int(((z >= 1e30).any(1) & ((z >= 20.0) & (z <= 3100.0)).any(1)).sum())
        err = nf.dbl_error(ref['points'][0, 2])
        print('mixed, camera %d: of %d blocks of 64 points %d mix z < 2 with z >= 2, %d z < 16 with z >= 16, %d z >= 1e30 with ordinary points; '
              'z-buffer: %d negative, %d below the band, %d empty under a weight'
              % (cam, z.shape[0], counts['2'], counts['16'], counts['1e30'], (ref['z_pre'] < 0).sum(), (~nf.in_band(ref['z_pre'])).sum(),
                 ((ref['z_pre'] == nf.EMPTY) & (ref['existing'] > 0)).sum()))
        assert min(counts.values()) >= 16
        assert (err[ref['points'][0, 2] >= nf.Z_CULL] < nf.BAND_LO).any() or cam == 2
    # the step forward keeps the near field, the step back crosses 2 and 16 downward
    z0, z1, z2 = (nf.oracle_frame(oracle, 'mixed', cam)['points'][0, 2] for cam in range(3))
    assert ((z0 < 2) & (z1 >= 2)).any() and ((z0 < 16) & (z1 >= 16)).any() and ((z0 >= 2) & (z2 < 2)).any() and ((z0 >= 16) & (z2 < 16)).any()
    assert (nf.oracle_frame(oracle, 'mixed', 1)['z_pre'] < 0).sum() >= 16


def test_dense_near_is_dense_and_a_fifth_of_it_near(oracle):
    cs = nf.case('dense_near')
    assert cs.points.shape[2] > 2 * cs.W * cs.H                 # csrc/kbe_frame.hip: p.dense
    for cam in frames_of('dense_near'):
        ref = nf.oracle_frame(oracle, 'dense_near', cam)
        err = nf.dbl_error(ref['points'][0, 2])
        share = float((err < nf.BAND_LO).mean())
        # lanes that merge their atomics: neighbours in the source raster's row with the same winner pixel, one of them outside the band
        w = ref['winner'].reshape(120, 128)
        e = err.reshape(120, 128)
        merged = (w[:, 0::2] == w[:, 1::2]) & (w[:, 0::2] >= 0) & ((e[:, 0::2] < nf.BAND_LO) != (e[:, 1::2] < nf.BAND_LO))
        negative_pairs = (w[:, 0::2] == w[:, 1::2]) & (w[:, 0::2] >= 0) & (e[:, 0::2] < 0) & (e[:, 1::2] < 0)
        print('dense_near, camera %d: %.3f of the points outside the band, %d pixels won by them (%d negative); %d pairs of row neighbours on one pixel '
              'with one of the two outside the band, %d with both negative'
              % (cam, share, (ref['z_pre'] < nf.BAND_LO).sum(), (ref['z_pre'] < 0).sum(), merged.sum(), negative_pairs.sum()))
        assert 0.17 < share < 0.23 and (ref['z_pre'] < 0).sum() >= 16 and ((ref['z_pre'] >= 0) & (ref['z_pre'] < nf.BAND_LO)).sum() >= 16
        assert merged.sum() >= 16 and negative_pairs.sum() >= 16
