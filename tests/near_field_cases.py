"""What tests/test_hip_near_field.py runs on: clouds whose depths leave the band in which the hot kernels' exact-arithmetic shortcuts
hold -- dblError = 1e6 - F*B / (z + 1e-7) (common.py:470) in [2^19, 1e6], i.e. z beyond F*B / 475712 (0.129 at F*B = 61440) -- each
built for what it crosses, and the two mutants that tests/test_near_field_cases.py holds them against.  Clouds are made in image-plane
coordinates (px = u * z / F), so every point is in view by construction.  Plain values and builders: nothing here needs a GPU."""
import collections

import numpy as np
import torch

FOCAL, BASELINE = 512.0, 120
FB = FOCAL * BASELINE
TILE_W, TILE_H = 32, 16                                     # csrc/kbe_tiles.h: KBE_TILE_W, KBE_TILE_H
BAND_LO, EMPTY = np.float32(524288.0), np.float32(1000000.0)        # csrc/kbe_device.h: degrid_fast_ok
Z_BAND = FB / (1000000.0 - 524288.0)                        # the depth whose dblError is 2^19: 0.12915...
Z_ZERO = FB / 1000000.0                                     # ... is 0: nearer points have negative dblError
Z_CULL = np.float32(0.001)                                  # common.py:453

# name, raster, points [1,3,N] / image [1,3,N] / depth [1,1,N] (CPU tensors), cameras [shift3] of fp32-representable floats, what it is there
# for, and prepare_cloud's `raster` (width, count) where the cloud is a row-major raster of another shape than W x H
Case = collections.namedtuple('Case', 'name W H points image depth cameras why raster')


def f32(v):
    return float(np.float32(v))


def tensor(a):
    """A reference array (read-only) as a tensor of its own."""
    return torch.from_numpy(np.array(a))


def dbl_error(z, fb=FB):
    """common.py:470 in fp64, rounded once."""
    return (1000000.0 - fb / (np.asarray(z, np.float32).astype(np.float64) + 0.0000001)).astype(np.float32)


def in_band(err):
    return (err >= BAND_LO) & (err <= EMPTY)


def _points(u, v, z):
    """Image-plane position (pixels from the optical axis) and depth -> camera-space points [3, N], fp32."""
    u, v, z = (np.asarray(a, np.float32) for a in (u, v, z))
    return np.stack([u * z / np.float32(FOCAL), v * z / np.float32(FOCAL), z]).astype(np.float32)


def _pixel_uv(x, y, W, H, dx=0.25, dy=0.25):
    """The image-plane position that projects to pixel (x, y) + (dx, dy): north-west corner (x, y), bilinear weight (1 - dx)(1 - dy) there."""
    return np.asarray(x, np.float32) - np.float32(0.5 * W - 0.5) + np.float32(dx), np.asarray(y, np.float32) - np.float32(0.5 * H - 0.5) + np.float32(dy)


def _raster(zr):
    """One point per pixel of a depth raster [H, W] (NaN: none), row-major."""
    H, W = zr.shape
    ys, xs = np.nonzero(~np.isnan(zr))
    u, v = _pixel_uv(xs, ys, W, H)
    return _points(u, v, zr[ys, xs])


def _case(name, W, H, pts, cameras, why, seed, permute=False, raster=None):
    rng = np.random.default_rng(seed)
    if permute:
        pts = pts[:, rng.permutation(pts.shape[1])]
    n = pts.shape[1]
    assert np.isfinite(pts).all()
    image = rng.random((1, 3, n), dtype=np.float32)
    depth = rng.uniform(100.0, 600.0, (1, 1, n)).astype(np.float32)        # the data channel the fill compares: unrelated to z, no ties
    cams = [tuple(f32(s) for s in cam) for cam in cameras]
    return Case(name, W, H, torch.from_numpy(np.ascontiguousarray(pts[None])), torch.from_numpy(image), torch.from_numpy(depth), cams, why, raster)


def _log_uniform(rng, lo, hi, n):
    return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)).astype(np.float32)


# ---------------------------------------------------------------------------------------
# edge19: the witnesses of the edge at 2^19
# ---------------------------------------------------------------------------------------

def edge_depths(edge=524288.0):
    """The consecutive fp32 depths whose dblError lies within 8 of `edge` (a power of two: the spacing of fp32 doubles there), found
    with the fp64 expression, and among their dblError values the pairs (a, c = fl32(a + 1.0f)) where the fp32 sum is NOT the fp64 one:
    `down` c < (double) a + 1.0 (fp32 says c >= a + 1, fp64 does not), `up` c > (double) a + 1.0 (fp32 says c <= a + 1, fp64 does not).
    -> (depths, their dblError, down [(z_a, z_c)], up [(z_a, z_c)])."""
    z0 = np.float32(FB / (1000000.0 - edge))
    z = (z0.view(np.uint32) + np.arange(-800, 801, dtype=np.int64)).astype(np.uint32).view(np.float32)
    err = dbl_error(z)
    keep = (err >= np.float32(edge - 8.0)) & (err <= np.float32(edge + 8.0))
    assert not keep[0] and not keep[-1], 'the window holds the whole run'
    z, err = z[keep], err[keep]
    depth_of = {}
    for zz, e in zip(z, err):
        depth_of.setdefault(float(e), zz)
    down, up = [], []
    for a in sorted(depth_of):
        c = float(np.float32(a) + np.float32(1.0))
        if c in depth_of and c != a + 1.0:
            (down if c < a + 1.0 else up).append((depth_of[a], depth_of[c]))
    return z, err, down, up


def edge19_depths():
    """edge_depths at the edge of the band, 2^19: depths around Z_BAND."""
    return edge_depths(float(BAND_LO))


def edge19():
    """96 x 64, one point per pixel, every dblError within 8 of 2^19.  Rows 0..31: columns alternate a, c of a `down` pair, so that
    every c lies between two a (and between a on its diagonals): fp64 keeps it, an fp32 comparison degrids it to a; no pair of the
    other neighbours (c above and below, all within 1 of one another) degrids anything.  Rows 32..63: depths drawn from the whole
    run (both sides of the edge in every wave), and on a 4-pixel grid a 3 x 3 block at a of an `up` pair -- its centre is degridded
    by nothing -- with a SECOND point on the centre at c: (1 - 0.25)^2 of its weight there, rejected by `c <= a + 1.0` in fp64, admitted in fp32."""
    W, H = 96, 64
    z, err, down, up = edge19_depths()
    assert len(down) >= 2 and len(up) >= 2
    rng = np.random.default_rng(19)
    zr = rng.choice(z, (H, W)).astype(np.float32)
    for y in range(32):
        za, zc = down[(y // 4) % len(down)]
        zr[y, 0::2], zr[y, 1::2] = za, zc
    extra_x, extra_y, extra_z = [], [], []
    for n, (gy, gx) in enumerate((gy, gx) for gy in range(34, 63, 4) for gx in range(2, 95, 4)):
        za, zc = up[n % len(up)]
        zr[gy - 1:gy + 2, gx - 1:gx + 2] = za
        extra_x.append(gx)
        extra_y.append(gy)
        extra_z.append(zc)
    u, v = _pixel_uv(extra_x, extra_y, W, H)
    pts = np.concatenate([_raster(zr), _points(u, v, extra_z)], 1)
    witnesses = np.zeros((H, W), bool)
    witnesses[extra_y, extra_x] = True
    case = _case('edge19', W, H, pts, [(0.0, 0.0, 0.0)], 'fp32 against fp64 comparisons at the edge of the band', 19)
    return case, witnesses


# ---------------------------------------------------------------------------------------
# band_tiles: where in tile + halo the value outside the band sits
# ---------------------------------------------------------------------------------------

BAND_TILES_NEAR = {                                          # raster -> the pixels (x, y) with a depth in [0.07, 0.12]
    (96, 64): [(x, y) for x in range(8, 13) for y in range(5, 10)]         # the interior of tile (0, 0)
              + [(31, y) for y in range(36, 44)]             # column 31 of tile (0, 2): tile (1, 2) sees it in its west halo only
              + [(31, 15)]                                   # the corner of tile (0, 0): halo of (1, 0) and (0, 1); of (1, 1) diagonally
              + [(95, 40), (70, 63)],                        # the image border (tiles (2, 2) and (2, 3))
    (50, 37): [(x, y) for x in range(44, 47) for y in range(33, 36)] + [(49, 36), (40, 20)],      # the partial tiles (1, 2) -- its corner too -- and (1, 1)
}
BAND_TILES_WITNESS = {(96, 64): (10, 7), (50, 37): (45, 34)}    # the centre of a 3 x 3 block of those pixels


def band_tiles(W=96, H=64):
    """An in-band background with values outside the band where BAND_TILES_NEAR says.  Most of what lies outside the band is harmless to
    the in-band arithmetic (c - 1.0f and a + 1.0f are exact away from a power of two), so a tile that wrongly took it would still be
    right; one 3 x 3 block is therefore a witness as edge19's, at an edge inside [0.07, 0.12], 2^17 (z = 0.0707): dblError a just
    below it, and a second point on the centre at c = fl32(a + 1.0f) > (double) a + 1.0.  (The halo classes are run against the oracle
    all the same; a wrong decision THERE has no such witness: the in-band degrid compares c - 1.0f, exact for every c in the band.)"""
    rng = np.random.default_rng(W)
    zr = rng.uniform(600.0, 1000.0, (H, W)).astype(np.float32)
    for x, y in BAND_TILES_NEAR[(W, H)]:
        zr[y, x] = rng.uniform(0.07, 0.12)
    za, zc = edge_depths(131072.0)[3][0]
    wx, wy = BAND_TILES_WITNESS[(W, H)]
    zr[wy - 1:wy + 2, wx - 1:wx + 2] = za
    assert 0.07 < za < 0.12 and 0.07 < zc < 0.12 and all((x, y) in BAND_TILES_NEAR[(W, H)] for x in range(wx - 1, wx + 2) for y in range(wy - 1, wy + 2))
    u, v = _pixel_uv([wx], [wy], W, H)
    pts = np.concatenate([_raster(zr), _points(u, v, [zc])], 1)
    name = 'band_tiles' if (W, H) == (96, 64) else 'band_tiles_%dx%d' % (W, H)
    return _case(name, W, H, pts, [(0.0, 0.0, 0.0)], 'the per-tile band decision over tile + halo', W)


def tile_band_classes(z_pre):
    """Per tile of a pre-degrid z-buffer [H, W], where its values outside the band are: 'inside' the tile, in the 'edge' of its
    one-pixel halo (E / W / N / S) only, in a 'diagonal' halo pixel only, or nowhere ('band').  -> {(tx, ty): class}"""
    H, W = z_pre.shape
    odd = np.zeros((H + 2, W + 2), bool)
    odd[1:-1, 1:-1] = ~in_band(z_pre)
    out = {}
    for ty in range(-(-H // TILE_H)):
        for tx in range(-(-W // TILE_W)):
            x0, y0 = tx * TILE_W, ty * TILE_H
            x1, y1 = min(x0 + TILE_W, W), min(y0 + TILE_H, H)
            box = odd[y0:y1 + 2, x0:x1 + 2]                  # tile + halo (the image's own border reads as in the band)
            inside = box[1:-1, 1:-1].any()
            edge = box[0, 1:-1].any() or box[-1, 1:-1].any() or box[1:-1, 0].any() or box[1:-1, -1].any()
            diagonal = box[0, 0] or box[0, -1] or box[-1, 0] or box[-1, -1]
            out[(tx, ty)] = 'inside' if inside else 'edge' if edge else 'diagonal' if diagonal else 'band'
    return out


# ---------------------------------------------------------------------------------------
# negative, far, mixed, dense_near
# ---------------------------------------------------------------------------------------

def _scattered(rng, n, W, H, z):
    """n points at random positions inside the raster."""
    return _points(rng.uniform(-0.5 * W + 0.5, 0.5 * W - 0.5, n), rng.uniform(-0.5 * H + 0.5, 0.5 * H - 0.5, n), z)


def negative():
    """An in-band raster (with two empty rectangles: holes for the fill) and, in random point order among it, points from the cull at
    z = 0.001 up to Z_ZERO and a little beyond: dblError from -6e7 through 0.  About a third of the pixels get one, some of them
    two (the order of two NEGATIVE keys), at random sub-pixel positions."""
    W, H = 96, 64
    rng = np.random.default_rng(61)
    zr = rng.uniform(20.0, 3000.0, (H, W)).astype(np.float32)
    zr[20:27, 60:75] = np.nan
    zr[50:60, 5:9] = np.nan
    n1 = int(0.35 * W * H)
    n2 = n1 // 2
    z_neg = np.concatenate([_log_uniform(rng, 0.001, 0.0614, n1 + n2), rng.uniform(0.0614, 0.0616, 200).astype(np.float32),
                            [Z_CULL, np.nextafter(Z_CULL, np.float32(0)), np.nextafter(Z_CULL, np.float32(1)), np.float32(Z_ZERO)]]).astype(np.float32)
    pts = np.concatenate([_raster(zr), _scattered(rng, z_neg.size, W, H, z_neg)], 1)
    cams = [(0.0, 0.0, 0.0), (1e-5, -2e-5, 0.004), (-2e-5, 1e-5, -0.0005)]
    return _case('negative', W, H, pts, cams, 'keys of negative dblError', 61, permute=True)


def far():
    """dblError == 1e6 exactly (z >= 2e6): columns 0..31 hold ONLY such points (the key stays KBE_ZKEY_EMPTY, the weight does not stay 0);
    columns 32..79 an ordinary point per pixel and such a point behind it; columns 80..95 a checkerboard of ordinary points and nothing
    (holes).  Among them points at 1e30..1e36 (project_xy: the wave leaves div_unscaled), which all project onto the optical axis."""
    W, H = 96, 64
    rng = np.random.default_rng(71)
    zr = np.full((H, W), np.nan, np.float32)
    zr[:, :32] = _log_uniform(rng, 2e6, 2e7, H * 32).reshape(H, 32)
    zr[:, 32:80] = rng.uniform(20.0, 3000.0, (H, 48))
    ys, xs = np.mgrid[0:H, 80:W]
    zr[:, 80:][(xs + ys) % 2 == 0] = rng.uniform(20.0, 3000.0, int(((xs + ys) % 2 == 0).sum()))
    behind_x, behind_y = rng.integers(32, 80, 1500), rng.integers(0, H, 1500)
    u, v = _pixel_uv(behind_x, behind_y, W, H, rng.random(1500), rng.random(1500))
    huge = np.concatenate([_log_uniform(rng, 1e30, 1e36, 12), _log_uniform(rng, 1e9, 1e20, 6), [np.float32(2e6), np.float32(1e36)]])
    pts = np.concatenate([_raster(zr), _points(u, v, _log_uniform(rng, 2e6, 2e7, 1500)), _scattered(rng, huge.size, W, H, huge)], 1)
    return _case('far', W, H, pts, [(0.0, 0.0, 0.0), (1.5, -0.75, -20.0)], 'dblError == 1e6, the empty key', 71, permute=True)


REGIMES = ('ordinary', 'unit', 'teens', 'near', 'negative', 'far', 'huge')


def _regime_depths(rng, regime, n):
    """n depths per point's regime: ordinary 20..3000; [0.5, 2) and [2, 20) (apply_shift's z + 1e-7f != z, project_err_fast's pz >= 16);
    near: outside the band, positive dblError; negative dblError; dblError == 1e6; 1e30..1e36."""
    draws = {'ordinary': rng.uniform(20.0, 3000.0, n), 'unit': rng.uniform(0.5, 2.0, n), 'teens': rng.uniform(2.0, 20.0, n),
             'near': rng.uniform(0.0615, 0.129, n), 'negative': _log_uniform(rng, 0.001, 0.0614, n), 'far': _log_uniform(rng, 2e6, 2e7, n),
             'huge': _log_uniform(rng, 1e30, 1e36, n)}
    z = np.zeros(n, np.float32)
    for k, name in enumerate(REGIMES):
        z[regime == k] = draws[name][regime == k]
    return z


def mixed():
    """Every point draws its regime by itself, so every wave of every route -- points by index, by raster patch, by Morton order -- mixes
    them.  Three cameras: none, a small step forward (z + sz crosses 2 and 16 upward; the near field stays in view), a step back (crosses
    them downward; the near field falls behind the cull)."""
    W, H = 96, 64
    rng = np.random.default_rng(83)
    n = 3 * W * H // 2
    regime = rng.choice(len(REGIMES), n, p=[0.44, 0.11, 0.11, 0.11, 0.11, 0.10, 0.02])
    pts = _scattered(rng, n, W, H, _regime_depths(rng, regime, n))
    cams = [(0.0, 0.0, 0.0), (1e-5, -2e-5, 0.01), (1.5, -0.75, -0.4)]
    return _case('mixed', W, H, pts, cams, 'every regime in every wave', 83)


def dense_near():
    """64 x 48 from a raster of 128 x 120 points, five per pixel (more than two: the z-splat pre-reduces within the wave -- a point with its
    neighbours in the row and in the next row of the source raster -- and merges their atomics), a fifth of them outside the band or negative."""
    W, H = 64, 48
    SW, SH = 128, 120
    rng = np.random.default_rng(97)
    n = SW * SH
    regime = rng.choice(len(REGIMES), n, p=[0.8, 0.0, 0.0, 0.1, 0.1, 0.0, 0.0])
    sy, sx = np.mgrid[0:SH, 0:SW]
    u = (sx.reshape(-1) + 0.5) * (W / SW) - 0.5 * W
    v = (sy.reshape(-1) + 0.5) * (H / SH) - 0.5 * H
    pts = _points(u, v, _regime_depths(rng, regime, n))
    return _case('dense_near', W, H, pts, [(0.0, 0.0, 0.0), (1e-7, -1e-7, 1e-5)], 'the dense z-splat on keys outside the band', 97, raster=(SW, n))


_CASES = {}


def case(name):
    """The case of a name, built once: tensors that no test writes to."""
    if not _CASES:
        e19, witnesses = edge19()
        for c in (e19, band_tiles(), band_tiles(50, 37), negative(), far(), mixed(), dense_near()):
            _CASES[c.name] = c
        _CASES['edge19', 'witnesses'] = witnesses
    return _CASES[name]


def edge19_witnesses():
    """[H, W] bool: the pixels of edge19 that hold a second point at c > (double) a + 1.0 behind their own at a."""
    case('edge19')
    return _CASES['edge19', 'witnesses']


NAMES = ['edge19', 'band_tiles', 'band_tiles_50x37', 'negative', 'far', 'mixed', 'dense_near']
BUILD_CASES = ['edge19', 'band_tiles', 'band_tiles_50x37']            # both forced builds of the fused tile launch
GROUP_CASES = ['mixed', 'negative']
MASK_CASES = ['negative', 'far', 'mixed']
FILL_CASES = ['far', 'negative']

_REFS = {}


def oracle_frame(oracle, name, cam):
    """Frame `cam` of a case by the CPU oracle (Jacobi schedule: the product's), stage by stage; rendered once, read-only."""
    if (name, cam) not in _REFS:
        cs = case(name)
        pts = oracle.shift_points(cs.points, torch.tensor(cs.cameras[cam], dtype=torch.float32))
        z0, winner = oracle.zsplat(pts, cs.W, cs.H, FOCAL, BASELINE, want_winner=True)
        zd = oracle.degrid(z0, 'jacobi')
        acc = oracle.accumulate(pts, torch.cat([cs.image, cs.depth], 1), zd, FOCAL, BASELINE)
        render, existing = oracle.normalize(acc)
        filled = oracle.fill_disocclusion(render, render[:, 3:4] * (existing > 0.0).float())
        ref = {'points': pts.numpy(), 'z_pre': z0.numpy()[0, 0], 'winner': winner.numpy()[0], 'z': zd.numpy()[0, 0], 'acc': acc.numpy(),
               'render': render.numpy()[0], 'existing': existing.numpy()[0, 0], 'filled': filled.numpy()[0], 'frame': oracle.frame_u8(filled[0])}
        for a in ref.values():
            a.setflags(write=False)
        _REFS[(name, cam)] = ref
    return _REFS[(name, cam)]


# ---------------------------------------------------------------------------------------
# the mutants
# ---------------------------------------------------------------------------------------

def degrid_restated(z, compare):
    """The Jacobi degrid (common.py:525-568) of a z-buffer [H, W] in numpy with its `c >= a + 1.0` comparisons in `compare`:
    np.float64 is the reference's arithmetic, np.float32 the mutant that a kernel off its exact branch would be."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    pad = np.full((H + 2, W + 2), np.nan, np.float32)
    pad[1:-1, 1:-1] = z
    c = z.astype(compare)
    one = compare(1.0)
    count = np.zeros((H, W), np.int32)
    total = np.zeros((H, W), np.float32)
    for ox, oy in ((1, 0), (0, 1), (1, 1), (1, -1)):         # :539-540
        a = pad[1 + oy:H + 1 + oy, 1 + ox:W + 1 + ox]
        d = pad[1 - oy:H + 1 - oy, 1 - ox:W + 1 - ox]
        with np.errstate(invalid='ignore'):
            use = ~np.isnan(a) & ~np.isnan(d) & (c >= a.astype(compare) + one) & (c >= d.astype(compare) + one)      # :548-557
        count += 2 * use
        total = (total + np.where(use, a, np.float32(0.0))).astype(np.float32)          # :559-560 (s + 0.0f == s)
        total = (total + np.where(use, d, np.float32(0.0))).astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = (total / count.astype(np.float32)).astype(np.float32)
    return np.where(count > 0, np.fmin(z, mean), z).astype(np.float32)                # :566


def fp32_ztest_zee(zee):
    """The z-buffer that makes the reference's `dblError <= zee + 1.0` (common.py:639, fp64) decide as the fp32 sum zee + 1.0f would:
    fl32(zee + 1.0f) - 1.0, which must itself be an fp32 value (asserted; it is around 2^19, where the two sums differ by 1/32)."""
    zee = np.asarray(zee, np.float32)
    limit = (zee + np.float32(1.0)).astype(np.float32)
    mutant = (limit.astype(np.float64) - 1.0).astype(np.float32)
    assert (mutant.astype(np.float64) + 1.0 == limit.astype(np.float64)).all(), 'the mutant z-buffer states the fp32 limit exactly'
    return mutant
