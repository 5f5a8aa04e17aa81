"""What tests/test_hip_intervals.py runs on, and the bar it holds every rendered value to: the EXACT normalised sum of a pixel and the
interval that every fp32 evaluation of it lies in.  tests/test_interval_cases.py holds the cases and the bar against the CPU oracle alone.

The bar.  Given the degridded z-buffer (held bit for bit on every route) the contributions to a pixel are a fixed set: n points with fp32
weights w_i >= 0 (common.py:481-484, bit for bit the reference's) and fp32 data d_i >= 0.  oracle.accumulate_exact sums d_i w_i and w_i in
fp64 -- the product of two fp32 values is exact there -- and divides: mean64 = S / (Wsum + (double) 1e-7f).  An fp32 evaluation, with
u = 2^-24:
  * forms each product with at most one rounding (a fused multiply-add: none): relative u;
  * adds n non-negative terms in any order, n - 1 roundings on the path of any term: together with the product (1 + u)^n, i.e. n u;
  * the weights the same, without the product: (n - 1) u; + 1e-7f (non-negative, one rounding): n u on the denominator;
  * divides with correct rounding: u.
So it lies within relative (2 n + 1) u, stated as (2 n + 2) u 1.0001 (second-order terms), of mean64 and its weight sum within
(n + 1) u 1.0001 of wsum64.  All terms are non-negative, so no cancellation widens it, and a value whose exact mean is 0 is exactly 0.
Nothing here is measured on the code under test.

Every colour is uint8 / 255, divided on the host as process_load does; the data's fourth channel is depth.  Plain values and builders:
nothing here needs a GPU."""
import collections

import numpy as np
import torch

FOCAL, BASELINE = 512.0, 120
U = 2.0 ** -24
SECOND_ORDER = 1.0001
# (focal, shift3): the identity; a step aside, up and forward; one focal of a dolly zoom (0.8 x 512: the image shrinks, the density grows)
CAMERAS = [(512.0, (0.0, 0.0, 0.0)), (512.0, (3.25, -1.5, -12.0)), (409.6, (1.0, -0.5, -24.0))]
PATCHES = ((200, 117, 33), (90, 90, 13), (255, 255, 255), (0, 0, 0))

# points [1,3,N] / image [1,3,N] / depth [1,1,N]: CPU tensors that no test writes to; raster: prepare_cloud's (width, count) hint or None
Case = collections.namedtuple('Case', 'name W H points image depth why raster')

NAMES = ['flat8', 'noise8', 'odd8', 'pile4', 'pile16', 'flat8_shuffled']
VIDEO_CASES = ['flat8', 'pile4']
FILL_CASES = ['flat8', 'noise8', 'odd8']


def tensor(a):
    """A reference array (read-only) as a tensor of its own."""
    return torch.from_numpy(np.array(a))


def colours_u8(rgb_u8):
    """uint8 [3, N] -> fp32 [1, 3, N], the division on the host (process_load)."""
    return torch.from_numpy((np.asarray(rgb_u8, np.uint8).astype(np.float32) / np.float32(255.0))[None])


def bump_disparity(W, H):
    """A smooth disparity bump: 60 outside a disc, 170 on it, a raised-cosine flank 1.5 pixels wide -- smooth, and steep enough that a
    step aside opens holes INSIDE the image (the parallax of the two levels differs by 3 pixels at the second camera)."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.hypot((xs - 0.45 * W) / 1.3, ys - 0.55 * H)
    t = np.clip((0.27 * H - r) / 1.5 + 0.5, 0.0, 1.0)
    return (60.0 + 110.0 * 0.5 * (1.0 - np.cos(np.pi * t))).astype(np.float32)


def _raster_case(oracle, name, W, H, rgb_u8, why, shuffle=None):
    disp = torch.from_numpy(bump_disparity(W, H))[None, None]
    depth = ((FOCAL * BASELINE) / (disp + 1e-7)).to(torch.float32)
    pts = oracle.depth_to_points(depth, FOCAL).reshape(1, 3, -1)
    image, depth = colours_u8(rgb_u8.reshape(3, -1)), depth.reshape(1, 1, -1)
    raster = None
    if shuffle is not None:
        order = torch.from_numpy(np.random.default_rng(shuffle).permutation(W * H))
        pts, image, depth = (t[:, :, order].contiguous() for t in (pts, image, depth))
        raster = (0, 0)                                         # no raster in front of this cloud
    return Case(name, W, H, pts, image, depth, why, raster)


def _flat_image(W, H):
    rgb = np.zeros((3, H, W), np.uint8)
    for by in range(-(-H // 24)):
        for bx in range(-(-W // 32)):
            rgb[:, by * 24:(by + 1) * 24, bx * 32:(bx + 1) * 32] = np.array(PATCHES[(bx + 2 * by + by // 2) % 4], np.uint8)[:, None, None]
    return rgb


def _noise_image(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, H, W), dtype=np.uint8)


def _pile_case(per_pixel):
    """test_pile_up_paths's cloud with 8-bit colours: 4 per pixel exceeds a tile's LDS record capacity (several insert-and-gather rounds),
    16 per pixel overflows the tile's bucket as well (the brute-force path)."""
    g0 = torch.Generator().manual_seed(per_pixel)
    W, H = 96, 64
    N = per_pixel * W * H
    u = torch.rand(N, generator=g0) * (W + 8) - 4 - W / 2 + 0.5
    v = torch.rand(N, generator=g0) * (H + 8) - 4 - H / 2 + 0.5
    z = torch.rand(N, generator=g0) * 400 + 600
    pts = torch.stack([u * z / 512.0, v * z / 512.0, z]).unsqueeze(0).contiguous()
    rgb = np.random.default_rng(per_pixel).integers(0, 256, (3, N), dtype=np.uint8)
    return Case('pile%d' % per_pixel, W, H, pts, colours_u8(rgb), z.view(1, 1, N).clone(), '%d points per pixel' % per_pixel, None)


_CASES = {}


def case(oracle, name):
    """The case of a name, built once (the unprojection is the oracle's)."""
    if not _CASES:
        flat = _flat_image(128, 96)
        for cs in (_raster_case(oracle, 'flat8', 128, 96, flat, 'flat 8-bit patches, one of them white, one black'),
                   _raster_case(oracle, 'noise8', 128, 96, _noise_image(128, 96, 8), '8-bit noise'),
                   _raster_case(oracle, 'odd8', 50, 37, _noise_image(50, 37, 37), 'partial tiles on both sides'),
                   _pile_case(4), _pile_case(16),
                   _raster_case(oracle, 'flat8_shuffled', 128, 96, flat, 'flat8 in a random point order', shuffle=5)):
            _CASES[cs.name] = cs
    return _CASES[name]


def data_of(cs):
    return torch.cat([cs.image, cs.depth], 1)


def point_orders(n):
    """Four orders of n points: as given, reversed, two random ones."""
    return [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(1).permutation(n), np.random.default_rng(2).permutation(n)]


# ---------------------------------------------------------------------------------------
# the exact reference of a frame and its intervals
# ---------------------------------------------------------------------------------------

_REFS = {}


def exact_frame(oracle, name, cam, extra=None):
    """Frame `cam` of a case: the z-buffers and the fp32 render of the oracle (Jacobi schedule: the product's) and the exact means,
    weight sums and counts on its z-buffer; computed once, read-only.  `extra` ([1, k, N]): further data channels (the tile renderer at
    7 channels), their exact means in 'mean64_extra'."""
    key = (name, cam, extra is not None)
    if key not in _REFS:
        cs = case(oracle, name)
        focal, shift3 = CAMERAS[cam]
        pts = oracle.shift_points(cs.points, torch.tensor(shift3, dtype=torch.float32))
        z0, _ = oracle.zsplat(pts, cs.W, cs.H, focal, BASELINE)
        zd = oracle.degrid(z0, 'jacobi')
        data = data_of(cs) if extra is None else torch.cat([data_of(cs), extra], 1)
        mean64, wsum64, n = oracle.accumulate_exact(pts, data, zd, focal, BASELINE)
        render, existing = oracle.normalize(oracle.accumulate(pts, data_of(cs), zd, focal, BASELINE))
        filled = oracle.fill_disocclusion(render, render[:, 3:4] * (existing > 0.0).float())
        ref = {'points': pts.numpy(), 'z_pre': z0.numpy()[0, 0], 'z': zd.numpy()[0, 0], 'mean64': mean64.numpy()[0], 'wsum64': wsum64.numpy()[0, 0],
               'n': n.numpy()[0, 0], 'render': render.numpy()[0], 'existing': existing.numpy()[0, 0], 'filled': filled.numpy()[0],
               'frame': oracle.frame_u8(filled[0]), 'covered': existing.numpy()[0, 0] > 0.0}
        assert np.array_equal(ref['covered'], ref['wsum64'] > 0.0)
        for a in ref.values():
            a.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def tolerance(n):
    """(relative tolerance of a normalised value, of the weight sum) of a pixel with n contributions."""
    n = np.asarray(n, np.float64)
    return (2.0 * n + 2.0) * U * SECOND_ORDER, (n + 1.0) * U * SECOND_ORDER


def interval_ratio(value, exact, tol, where):
    """max over `where` of |value - exact| / (tol * exact); a value whose exact one is 0 must be 0 (else inf).  value [..., H, W] fp32,
    exact the same shape fp64, tol and where [H, W]."""
    value, exact = np.asarray(value, np.float64), np.asarray(exact, np.float64)
    where = np.broadcast_to(where, value.shape)
    tol = np.broadcast_to(tol, value.shape)
    err = np.abs(value - exact)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(exact > 0.0, err / (tol * exact), np.where(err > 0.0, np.inf, 0.0))
    return np.where(where, ratio, 0.0)


def check_intervals(render, existing, ref, what, exact=None):
    """(a) of the bar: every channel of `render` [C,H,W] inside its interval at every covered pixel, `existing` [H,W] inside its own,
    the covered set the oracle's.  -> (worst ratio of the values, of the weights)."""
    exact = ref['mean64'] if exact is None else exact
    render, existing = np.asarray(render), np.asarray(existing)
    assert render.dtype == np.float32 and existing.dtype == np.float32 and render.shape == exact.shape
    assert np.array_equal(existing > 0.0, ref['covered']), what + ': the covered set'
    tol_v, tol_w = tolerance(ref['n'])
    rv = interval_ratio(render, exact, tol_v, ref['covered'])
    rw = interval_ratio(existing, ref['wsum64'], tol_w, ref['covered'])
    for r, which in ((rv, 'value'), (rw, 'weight sum')):
        if not (r <= 1.0).all():
            worst = np.unravel_index(np.argmax(r), r.shape)
            y, x = worst[-2:]
            raise AssertionError('%s: %s %s leaves its interval: %.3f of the tolerance (n = %d); %d values outside'
                                 % (what, which, worst, r[worst], ref['n'][y, x], (r > 1.0).sum()))
    return float(rv.max()), float(rw.max())


def u8_of(x):
    """common.py:255 on fp32 values: fp32 product, clip, truncation."""
    return np.clip(np.asarray(x, np.float32) * np.float32(255.0), np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def legal_bytes(ref):
    """The legal byte set of every colour value, {(uint8) trunc(255 x) : x an fp32 value in the interval, clipped}: to_u8 is monotone, so
    it is the range between the bytes of the interval's smallest and largest fp32 value.  -> (lo, hi) uint8 [H, W, 3]."""
    tol = tolerance(ref['n'])[0][None]
    m = ref['mean64'][:3]
    lo64, hi64 = m * (1.0 - tol), m * (1.0 + tol)
    lo, hi = lo64.astype(np.float32), hi64.astype(np.float32)
    lo = np.where(lo.astype(np.float64) < lo64, np.nextafter(lo, np.float32(np.inf)), lo)
    hi = np.where(hi.astype(np.float64) > hi64, np.nextafter(hi, np.float32(-np.inf)), hi)
    assert (lo <= hi).all(), 'an interval of relative width >= 4 u holds an fp32 value'
    return u8_of(lo).transpose(1, 2, 0), u8_of(hi).transpose(1, 2, 0)


def check_bytes(frame, ref, what):
    """Every byte of a covered pixel in its legal set.  -> the share of bytes whose set has two members."""
    lo, hi = legal_bytes(ref)
    frame = np.asarray(frame)
    cov = ref['covered'][:, :, None]
    bad = cov & ((frame < lo) | (frame > hi))
    assert not bad.any(), '%s: %d bytes outside their legal set, the first at %s' % (what, bad.sum(), np.argwhere(bad)[0])
    assert (hi - lo <= 1).all()
    return float(((hi > lo) & cov).mean())


def fill_of(oracle, render, existing):
    """oracle.fill_disocclusion of an UNFILLED float render [4,H,W] under the hole mask common.py:253 makes of it."""
    r = torch.from_numpy(np.ascontiguousarray(render))[None]
    e = torch.from_numpy(np.ascontiguousarray(existing)).reshape(1, 1, *render.shape[1:])
    return oracle.fill_disocclusion(r, r[:, 3:4] * (e > 0.0).float()).numpy()[0]


def filled_bytes(oracle, frame, ref, depth=None):
    """A frame [H,W,3] uint8 with its holes filled anew: oracle.fill_disocclusion of its own bytes (holes zeroed) under the oracle's
    hole mask and `depth` (default: the exact depth, rounded once) -- what a frame of which only bytes come out is held against."""
    depth = ref['mean64'][3].astype(np.float32) if depth is None else depth
    x = np.where(ref['covered'][None], np.asarray(frame).transpose(2, 0, 1).astype(np.float32), np.float32(0.0))
    d = np.where(ref['covered'], depth, np.float32(0.0)).astype(np.float32)
    out = oracle.fill_disocclusion(torch.from_numpy(np.ascontiguousarray(x))[None], torch.from_numpy(d)[None, None]).numpy()[0]
    return out.astype(np.uint8).transpose(1, 2, 0)


def psnr(a, b, peak=1.0):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 200.0 if mse == 0 else 10.0 * np.log10(peak * peak / mse)


# ---------------------------------------------------------------------------------------
# the mutant
# ---------------------------------------------------------------------------------------

def dropping_mutant(oracle, name, cam, below):
    """The exact means of a frame without every contribution whose weight is below `below` of its pixel's exact weight sum: what a
    gather that loses small-weight records would compute.  -> (mean64 [4,H,W], wsum64 [H,W])."""
    cs, ref = case(oracle, name), exact_frame(oracle, name, cam)
    focal, _ = CAMERAS[cam]
    mean64, wsum64, _ = oracle.accumulate_exact(tensor(ref['points']), data_of(cs), tensor(ref['z'])[None, None], focal, BASELINE,
                                                drop_below=(tensor(ref['wsum64']), below))
    return mean64.numpy()[0], wsum64.numpy()[0, 0]
