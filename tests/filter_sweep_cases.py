"""What tests/test_filter_sweeps.py (CPU) and tests/test_filter_sweeps_gpu.py share: the parameters of the sweeps over the five tile
filters (kbe_area_reduce_u8, kbe_crop_area_u8, kbe_dof_u8, kbe_enlarge_u8, kbe_sharpen_u8), the alignment classes those parameters reach --
computed from the kernels' launch arithmetic alone --, an exact area reduction that needs no weight matrix, for the sides' limit, and the
frames that make a radius visible.

The code the sweeps are about is not in the *_block.h headers and exists once per kernel (csrc/kbe_area.hip, kbe_crop_area.hip, kbe_dof.hip,
kbe_enlarge.hip, kbe_sharpen.hip):
  the tile store    a tile's row of nx <= 64 pixels is put together in LDS `lead` = (its address mod 16) bytes into an LDS row and written as
                    16-byte pieces, dwords and single bytes: its class is (lead, nx), 16 x 64 of them;
  the row fetch     a staged row of `len` pixels is fetched as the aligned dwords from `shift` = (its address & 3) bytes before it,
                    (shift + 3 len + 3) >> 2 of them: its class is (shift, 3 len mod 4), 4 x 4 of them;
  sharpen's halo    a staged row lies behind a left halo of `left` pixels that the frame does not have, rounded up to a dword, and `shift`
                    bytes on; `right` pixels are repeated behind it.  left is 0 or R: its class is (shift, R, which borders, right);
  enlarge's LDS row a raw row of up to 68 pixels at a shift of up to 3 fills the 52 dwords an LDS row has, and up to 20 rows are staged."""
import functools

import numpy as np

import area_cases as ac
import crop_area_cases as cc
import dof_cases as dc
import enlarge_cases as ec
import gif_cases as gc
import sharpen_cases as sc

# -- the kernels' layout, as far as the classes depend on it -------------------------------------
TILE_X = 64
TILE_Y = {'area': 4, 'crop_area': 4, 'dof': 16, 'enlarge': 16, 'sharpen': 32}        # kTileY
STRIP_ROWS, STRIP_PX = 16, {'area': 340, 'crop_area': 339}         # kStripRows, kStripPx: a strip of the source (of the patch)
ALLOCATION = 512                                                   # every allocation starts on a multiple of it (tests/guarded.py); the GPU tests assert it

RAW_PX, RAW_ROWS = TILE_X + 4, TILE_Y['enlarge'] + 4               # enlarge's kRawPx, kRawRows: the taps of 64 (16) targets and the second taps
MAX_RADIUS = 24                                                    # sharpen's kMaxRadius

EVERY_STORE_CLASS = frozenset((lead, nx) for lead in range(16) for nx in range(1, TILE_X + 1))
EVERY_FETCH_CLASS = frozenset((shift, rest) for shift in range(4) for rest in range(4))


def store_classes(w, h, out_stride, shift=0):
    """{(lead, nx)} of an output of w x h pixels, its rows out_stride bytes apart, `shift` bytes off its allocation: the same for the five
    kernels -- a tile is 64 pixels across in all of them, and a tile's row starts 192 bytes after its left neighbour's."""
    assert ALLOCATION % 16 == 0
    return {((shift + oy * out_stride + 3 * ox0) % 16, min(TILE_X, w - ox0)) for oy in range(h) for ox0 in range(0, w, TILE_X)}


def _spans(N, n, tile):
    """[begin, end) of the sources under each tile of `tile` targets of an axis: span_begin of its first, span_end of its last (kbe_area_block.h)."""
    return [(o0 * N // n, ((o0 + min(tile, n - o0)) * N + n - 1) // n) for o0 in range(0, n, tile)]


def _pieces(begin, end, step):
    return [(a, min(a + step, end)) for a in range(begin, end, step)]


def _row_class(at, length):
    return at % 4, 3 * length % 4


def area_fetch_classes(W, H, w, h, stride, src_shift):
    """{(shift, 3 len mod 4)} of k_area_reduce: per tile the strips of its span, per strip its rows, from pixel x0 on."""
    found = set()
    for x_begin, x_end in _spans(W, w, TILE_X):
        for y_begin, y_end in _spans(H, h, TILE_Y['area']):
            for x0, x1 in _pieces(x_begin, x_end, STRIP_PX['area']):
                found |= {_row_class(src_shift + sy * stride + 3 * x0, x1 - x0) for sy in range(y_begin, y_end)}
    return found


def crop_area_fetch_classes(W, H, crop, size, stride, src_shift):
    """{(shift, 3 len mod 4)} of k_crop_area: under a strip of the patch its raw rectangle, one pixel and one row more where the crop starts on a
    half pixel, as far as the frame goes."""
    (cw, ch), (w, h) = crop, size
    (ipx, hx), (ipy, hy) = cc.start(W, cw), cc.start(H, ch)
    found = set()
    for x_begin, x_end in _spans(cw, w, TILE_X):
        for y_begin, y_end in _spans(ch, h, TILE_Y['crop_area']):
            for y0, y1 in _pieces(y_begin, y_end, STRIP_ROWS):
                for x0, x1 in _pieces(x_begin, x_end, STRIP_PX['crop_area']):
                    rx0, rx1 = ipx + x0, min(ipx + x1 + hx, W)
                    found |= {_row_class(src_shift + ry * stride + 3 * rx0, rx1 - rx0) for ry in range(ipy + y0, min(ipy + y1 + hy, H))}
    return found


def dof_fetch_classes(W, H, R, stride, src_shift):
    """{(shift, 3 len mod 4)} of k_dof: a tile and its halo of R pixels, as far as the frame goes."""
    found = set()
    for ox0 in range(0, W, TILE_X):
        fx0, fx1 = max(ox0 - R, 0), min(ox0 + min(TILE_X, W - ox0) + R, W)
        for oy0 in range(0, H, TILE_Y['dof']):
            fy0, fy1 = max(oy0 - R, 0), min(oy0 + min(TILE_Y['dof'], H - oy0) + R, H)
            found |= {_row_class(src_shift + fy * stride + 3 * fx0, fx1 - fx0) for fy in range(fy0, fy1)}
    return found


def _sharpen_tiles(W, R):
    """(fx, lx, left, right) of k_sharpen's tiles across: the frame's pixels [fx, lx) are staged, `left` and `right` pixels of the tile's halo
    of R lie beyond the frame."""
    for x0 in range(0, W, TILE_X):
        nx = min(TILE_X, W - x0)
        fx, lx = max(x0 - R, 0), min(x0 + nx + R, W)
        yield fx, lx, fx + R - x0, x0 + nx + R - lx


def _sharpen_rows(H, R):
    """The frame rows of k_sharpen's staged rows, tile row by tile row: staged row r of the tile at y0 is frame row clamp(y0 - R + r)."""
    for y0 in range(0, H, TILE_Y['sharpen']):
        ny = min(TILE_Y['sharpen'], H - y0)
        yield [min(max(y0 - R + r, 0), H - 1) for r in range(ny + 2 * R)]


def sharpen_fetch_classes(W, H, R, stride, src_shift):
    """{(shift, 3 span mod 4)} of k_sharpen: per tile its pixels and up to R more on either side, as far as the frame goes, of every staged row
    -- the rows beyond the frame are the border rows again."""
    found = set()
    for fx, lx, _, _ in _sharpen_tiles(W, R):
        for rows in _sharpen_rows(H, R):
            found |= {_row_class(src_shift + fy * stride + 3 * fx, lx - fx) for fy in rows}
    return found


def sharpen_stage_classes(W, H, R, stride, src_shift):
    """{(shift, R, border)} of k_sharpen's staged rows; border: 'neither', 'left', ('right', right) or ('both', right) -- which of the
    tile's halos lie beyond the frame, and by how many pixels the right one does.  (The left one does by R or not at all: a tile starts at a
    multiple of 64 > R.)"""
    found = set()
    for fx, lx, left, right in _sharpen_tiles(W, R):
        assert left in (0, R) and 0 <= right <= R
        border = (('both', right) if right else 'left') if left else (('right', right) if right else 'neither')
        for rows in _sharpen_rows(H, R):
            found |= {((src_shift + fy * stride + 3 * fx) % 4, R, border) for fy in rows}
    return found


def _enlarge_spans(n_in, n_out, tile):
    """[p0, p1) of the patch under each tile of `tile` targets of an axis: the first tap of its first target to the last tap of its last, both
    clamped (enlarge_cases.axis)."""
    taps = ec.axis(n_in, n_out)[1]
    return [(int(taps[o0, 0]), int(taps[min(o0 + tile, n_out) - 1, 3]) + 1) for o0 in range(0, n_out, tile)]


def enlarge_cuts(n_in, n_out, tile):
    """[(whether the clamp at the patch's first pixel cuts the tile's span, whether the one at its last pixel does)] per tile of an axis, from
    the positions themselves: i = floor(((2 x + 1) n_in - n_out) / (2 n_out)), the taps i - 1 .. i + 2."""
    at = lambda x: ((2 * x + 1) * n_in - n_out) // (2 * n_out)                     # noqa: E731
    return [(at(o0) - 1 < 0, at(min(o0 + tile, n_out) - 1) + 2 > n_in - 1) for o0 in range(0, n_out, tile)]


def enlarge_fetch_classes(W, H, crop, size, stride, src_shift):
    """({(shift, 3 len mod 4)}, the largest (len, shift), the most rows a tile stages) of k_enlarge: under a tile's span of the patch its raw
    rectangle, one pixel and one row more where the crop starts on a half pixel, as far as the frame goes."""
    (cw, ch), (w, h) = crop, size
    (ipx, hx), (ipy, hy) = cc.start(W, cw), cc.start(H, ch)
    found, longest, most = set(), (0, 0), 0
    for px0, px1 in _enlarge_spans(cw, w, TILE_X):
        for py0, py1 in _enlarge_spans(ch, h, TILE_Y['enlarge']):
            rx0, rx1 = ipx + px0, min(ipx + px1 + hx, W)
            ry0, ry1 = ipy + py0, min(ipy + py1 + hy, H)
            for ry in range(ry0, ry1):
                at = src_shift + ry * stride + 3 * rx0
                found.add(_row_class(at, rx1 - rx0))
                longest = max(longest, (rx1 - rx0, at % 4))
            most = max(most, ry1 - ry0)
    return found, longest, most


def odd_pad(pixels):
    """1 or 2: what makes rows of `pixels` 3-byte pixels an odd number of bytes apart, so that 16 rows take every address mod 16 (4: mod 4)."""
    return 2 if pixels % 2 else 1


# -- the store sweep -----------------------------------------------------------------------------
# one tile across at every width it can have; then a second tile 192 bytes on -- the same lead -- that is 1, 63 and 64 wide, and a third
STORE_WIDTHS = tuple(range(1, TILE_X + 1)) + (65, 127, 128, 129)
STORE_ROWS = 16                                                    # with an odd stride: every lead
COPY_WIDTHS = (1, 2, 5, 11, 16, 21, 43, 48, 63, 64, 65, 129)       # area at ratio 1
SOURCE_ROWS = 37                                                   # 37 -> 16 rows: no integer ratio
# area: 'ratio' 2 w + 1 -> w (no integer but at w = 1, which has none) and 37 -> 16, 'copy' w x 16 as it is;  crop_area: the crop 2 w + 1 x 37 that
# starts on whole pixels on both axes (the staged raw rows are the patch) and on half pixels on both;  dof: the caps 16 and 3
# enlarge: the crop (2 w + 2) // 3 x 11 -> w x 16 that starts on whole pixels on both axes (the pass along the rows reads the staged raw rows)
# and on half pixels on both (it reads the patch);  sharpen: a radius whose halo is a dword and a half, and the largest
STORE_SWEEPS = [('area', 'ratio'), ('area', 'copy'), ('crop_area', 'oo'), ('crop_area', 'ee'), ('dof', 16), ('dof', 3),
                ('enlarge', 'oo'), ('enlarge', 'ee'), ('sharpen', 2), ('sharpen', 24)]
DOF_FOCUS, DOF_APERTURE = 100.0, 16.0
# widths of their own that are taller than STORE_ROWS, {width: rows}: three tiles across and three (two) down -- enlarge's second band of tile
# rows 0 .. 15 and a third that is cut, sharpen's trips over tile rows 16 .. 31 and a second band
TALL = {'enlarge': {130: 40}, 'sharpen': {130: 40}}
ENLARGE_CROP_ROWS = {STORE_ROWS: 11, 40: 27}
SHARPEN_AMOUNT = 512


def store_widths(entry, variant):
    return COPY_WIDTHS if (entry, variant) == ('area', 'copy') else STORE_WIDTHS + tuple(TALL.get(entry, ()))


def store_rows(entry, w):
    return TALL.get(entry, {}).get(w, STORE_ROWS)


def radius_taps(R):
    """sharpen_cases.taps_of at a sigma whose radius is R: (w_0, .., w_R)."""
    sigma = (R - 0.1) / 3.0
    assert sc.radius_of(sigma) == R
    return sc.taps_of(sigma)


def store_stride(w):
    return 3 * w + odd_pad(w)


def sweep_depth(W, H):
    """[1, H, W] depths 50 .. 106 that repeat every 9 pixels along a row and shift by 2 from row to row: at DOF_FOCUS and DOF_APERTURE radii from
    0 to 16 side by side, some above 0 in every tile."""
    y, x = np.mgrid[0:H, 0:W]
    return (50.0 + 7.0 * ((x + 2 * y) % 9)).astype(np.float32)[None]


@functools.lru_cache(maxsize=None)
def store_case(entry, variant, w):
    """(the call's arguments after the module: a tuple, its keywords, the twin's bytes [1, 16, w, 3]) of one width of a store sweep."""
    h, kw = store_rows(entry, w), dict(pad=1, out_pad=odd_pad(w))
    if entry == 'enlarge':
        crop = ((2 * w + 2) // 3, ENLARGE_CROP_ROWS[h])
        frames = gc.photo_like(crop[1] + cc.OFF[variant][1], crop[0] + cc.OFF[variant][0], 7 + w)[None]
        assert (cc.start(frames.shape[2], crop[0])[1], cc.start(frames.shape[1], crop[1])[1]) == {'oo': (False, False), 'ee': (True, True)}[variant]
        return (frames, crop, (w, h)), kw, ec.twin_enlarge(frames, crop, (w, h))
    if entry == 'sharpen':
        frames, taps = gc.photo_like(h, w, 7 + w)[None], radius_taps(variant)
        return (frames, taps, SHARPEN_AMOUNT), kw, sc.twin_sharpen(frames, taps, SHARPEN_AMOUNT)
    if entry == 'area':
        frames = gc.photo_like(h, w, 7 + w)[None] if variant == 'copy' else gc.photo_like(SOURCE_ROWS, 2 * w + 1, 7 + w)[None]
        return (frames, w, h), kw, ac.twin_reduce(frames, w, h)
    if entry == 'crop_area':
        crop = (2 * w + 1, SOURCE_ROWS)
        frames = gc.photo_like(crop[1] + cc.OFF[variant][1], crop[0] + cc.OFF[variant][0], 7 + w)[None]
        assert (cc.start(frames.shape[2], crop[0])[1], cc.start(frames.shape[1], crop[1])[1]) == {'oo': (False, False), 'ee': (True, True)}[variant]
        return (frames, crop, (w, h)), kw, cc.twin_reduce(frames, crop, (w, h))
    frames, depth = gc.photo_like(h, w, 7 + w)[None], sweep_depth(w, h)
    radii = dc.twin_radius(depth[0], DOF_FOCUS, DOF_APERTURE, variant)
    assert all(radii[:, x0:x0 + TILE_X].max() > 0 for x0 in range(0, w, TILE_X)) and radii.min() == 0            # a radius above 0 in every tile
    return (frames, depth, [DOF_FOCUS], DOF_APERTURE, variant), kw, dc.twin_blur(frames, depth, [DOF_FOCUS], DOF_APERTURE, variant)


def store_sweep_classes(entry, variant):
    """The (lead, nx) classes a store sweep reaches: from its widths and strides alone, the outputs on their allocations' starts."""
    found = set()
    for w in store_widths(entry, variant):
        found |= store_classes(w, store_rows(entry, w), store_stride(w))
    return found


# -- the fetch sweep -----------------------------------------------------------------------------
SRC_SHIFTS = (0, 1, 2, 3)
FETCH_SWEEPS = [('area', None), ('crop_area', 'oo'), ('crop_area', 'ee'), ('dof', 16), ('enlarge', 'oo'), ('enlarge', 'ee'), ('sharpen', 7)]
# four consecutive widths: every 3 len mod 4.  area, crop_area: a strip of 340 (339) pixels and a shorter one in the first tile, a second tile
# that starts elsewhere; dof: two tiles, the second one's window starts 48 pixels in; enlarge: the crop's width, two tiles whose spans the
# patch's borders cut; sharpen: two tiles, the second one's rows start 57 pixels in
FETCH_WIDTHS = {'area': (380, 381, 382, 383), 'crop_area': (371, 372, 373, 374), 'dof': (69, 70, 71, 72), 'enlarge': (69, 70, 71, 72), 'sharpen': (69, 70, 71, 72)}
FETCH_ROWS = {'area': 9, 'crop_area': 9, 'dof': 7, 'enlarge': 9, 'sharpen': 7}
FETCH_TARGET = (70, 5)


def enlarge_fetch_target(W, H):
    """(w, h) of the enlargement of a crop W x H in the fetch sweep: no integer ratio on either axis."""
    return W + 9, H + 4


def fetch_stride(W):
    return 3 * W + odd_pad(W)


@functools.lru_cache(maxsize=None)
def fetch_case(entry, variant, W):
    """(arguments, keywords without src_shift, the twin's bytes) of one width of a fetch sweep; W: the width of what is fetched from -- the
    source, the crop, the frame."""
    H, kw = FETCH_ROWS[entry], dict(out_pad=3)
    if entry == 'enlarge':
        crop, size = (W, H), enlarge_fetch_target(W, H)
        frames = gc.photo_like(H + cc.OFF[variant][1], W + cc.OFF[variant][0], 3 + W)[None]
        return (frames, crop, size), dict(kw, pad=odd_pad(frames.shape[2])), ec.twin_enlarge(frames, crop, size)
    if entry == 'sharpen':
        frames, taps = gc.photo_like(H, W, 3 + W)[None], radius_taps(variant)
        return (frames, taps, SHARPEN_AMOUNT), dict(kw, pad=odd_pad(W)), sc.twin_sharpen(frames, taps, SHARPEN_AMOUNT)
    if entry == 'area':
        frames = gc.photo_like(H, W, 3 + W)[None]
        return (frames,) + FETCH_TARGET, dict(kw, pad=odd_pad(W)), ac.twin_reduce(frames, *FETCH_TARGET)
    if entry == 'crop_area':
        crop = (W, H)
        frames = gc.photo_like(H + cc.OFF[variant][1], W + cc.OFF[variant][0], 3 + W)[None]
        return (frames, crop, FETCH_TARGET), dict(kw, pad=odd_pad(frames.shape[2])), cc.twin_reduce(frames, crop, FETCH_TARGET)
    frames, depth = gc.photo_like(H, W, 3 + W)[None], sweep_depth(W, H)
    return (frames, depth, [DOF_FOCUS], DOF_APERTURE, variant), dict(kw, pad=odd_pad(W)), dc.twin_blur(frames, depth, [DOF_FOCUS], DOF_APERTURE, variant)


def fetch_sweep_classes(entry, variant):
    """The (shift, 3 len mod 4) classes a fetch sweep reaches: from its shapes, strides and shifts alone."""
    found = set()
    for W in FETCH_WIDTHS[entry]:
        H = FETCH_ROWS[entry]
        for src_shift in SRC_SHIFTS:
            if entry == 'area':
                found |= area_fetch_classes(W, H, *FETCH_TARGET, fetch_stride(W), src_shift)
            elif entry == 'crop_area':
                FW, FH = W + cc.OFF[variant][0], H + cc.OFF[variant][1]
                found |= crop_area_fetch_classes(FW, FH, (W, H), FETCH_TARGET, fetch_stride(FW), src_shift)
            elif entry == 'enlarge':
                FW, FH = W + cc.OFF[variant][0], H + cc.OFF[variant][1]
                found |= enlarge_fetch_classes(FW, FH, (W, H), enlarge_fetch_target(W, H), fetch_stride(FW), src_shift)[0]
            elif entry == 'sharpen':
                found |= sharpen_fetch_classes(W, H, variant, fetch_stride(W), src_shift)
            else:
                found |= dof_fetch_classes(W, H, variant, fetch_stride(W), src_shift)
    return found


# -- sharpen at every radius ---------------------------------------------------------------------
SHARPEN_RADII = tuple(range(1, MAX_RADIUS + 1))
# taps that do not fall with the distance and add up to 32768 = 20000 + 2 (1000 + 5000 + 384): a tap taken at another distance shows
ODD_TAPS = (20000, 1000, 5000, 384)


def sharpen_radius_frames(R):
    """[(W, H)] of the frames of a radius, each with H >= 4 rows an odd number of bytes apart, so that every tile stages rows at every shift:
      three tiles whose middle one has its whole halo inside the frame, the first one's left halo and the last one's right halo -- all R of
      it -- beyond it;
      from R = 2 on, three tiles whose last is m < R wide: the middle one's right halo lies R - m pixels beyond the frame (0 < right < R);
      one tile narrower than 64: both halos beyond the frame.
    From R = 5 on the frames have fewer rows than R: every staged row above and below the tile is a border row again."""
    wide = (2 * TILE_X + R + 1 + R % 3, 5 + R % 4)
    cut = [(2 * TILE_X + 1 + (R // 2 + 3 * (R % 5)) % (R - 1), 4)] if R >= 2 else []
    return [wide] + cut + [(1 + 5 * R % 63, 7)]


@functools.lru_cache(maxsize=None)
def sharpen_radius_case(R, frame, taps=None):
    """(arguments, keywords, the twin's bytes) of one frame of a radius: the source R mod 4 bytes off its allocation."""
    W, H = frame
    frames, taps = gc.photo_like(H, W, 11 + R + W)[None], taps or radius_taps(R)
    assert len(taps) == R + 1
    kw = dict(pad=odd_pad(W), out_pad=odd_pad(W), src_shift=R % 4)
    return (frames, taps, SHARPEN_AMOUNT), kw, sc.twin_sharpen(frames, taps, SHARPEN_AMOUNT)


def sharpen_radius_classes(R):
    found = set()
    for W, H in sharpen_radius_frames(R):
        found |= sharpen_stage_classes(W, H, R, fetch_stride(W), R % 4)
    return found


# -- enlarge at a full LDS row -------------------------------------------------------------------
# (frame, crop, size), W x H each.  190 targets from 189 sources: the 64 targets of the middle tile lie at 63 .. 126, 64 positions in a row,
# so their taps are the 67 patch pixels 62 .. 128; 46 from 45: the middle band's 16 targets lie at 15 .. 30, their taps are the 19 rows
# 14 .. 32.  The first crop starts on half pixels on both axes: 68 raw pixels and 20 raw rows, which is all an LDS row and the staged
# rectangle hold; the second on whole pixels: the pass along the rows reads the staged raw rows, 67 pixels of 19 rows.  In both the first
# and the last tile's and band's span is cut by the clamp at the patch's border.
FULL_ROWS = [((191, 47), (189, 45), (190, 46)), ((192, 48), (189, 45), (190, 46))]


@functools.lru_cache(maxsize=None)
def full_row_case(i):
    """(arguments, keywords without src_shift, the twin's bytes) of FULL_ROWS[i]."""
    (W, H), crop, size = FULL_ROWS[i]
    frames = gc.photo_like(H, W, 31 + i)[None]
    return (frames, crop, size), dict(pad=odd_pad(W), out_pad=odd_pad(size[0])), ec.twin_enlarge(frames, crop, size)


# -- an exact area reduction without a weight matrix ------------------------------------------------
def _along(a, n):
    """int64 [N, ...] -> [n, ...]: the weighted sums of kbe_area_block.h along the first axis.  On the axis of N n units source s covers
    [s n, (s + 1) n); F(t), the integral of the sources over [0, t), is n P[t div n] + (t mod n) v[t div n] with P the sources' prefix sums,
    and target o, which covers [o N, (o + 1) N), gets F((o + 1) N) - F(o N)."""
    N = a.shape[0]
    assert a.dtype == np.int64 and 1 <= n <= N
    zero = np.zeros((1,) + a.shape[1:], np.int64)
    P, v = np.concatenate([zero, np.cumsum(a, axis=0)]), np.concatenate([a, zero])           # (t = N n: P[N], and no part of a source beyond it)
    q, r = np.divmod(np.arange(n + 1, dtype=np.int64) * N, n)
    F = n * P[q] + r.reshape((-1,) + (1,) * (a.ndim - 1)) * v[q]
    return np.diff(F, axis=0)


def exact_reduce(frames, w, h):
    """uint8 [..., H, W, 3] -> uint8 [..., h, w, 3]: S by prefix sums along x, then along y, in int64 (S <= 255 W H, and on the way
    h (255 W H) < 2^63), then (2 S + W H) // (2 W H).  Independent of area_cases.twin_reduce, and it works at any size."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    H, W = a.shape[-3], a.shape[-2]
    a = np.moveaxis(a.astype(np.int64), (-3, -2), (1, 0))                # [W, H, ..., 3]
    S = np.swapaxes(_along(np.swapaxes(_along(a, w), 0, 1), h), 0, 1)      # [w, h, ..., 3]
    S = np.moveaxis(S, (1, 0), (-3, -2))
    return ((2 * S + W * H) // (2 * W * H)).astype(np.uint8)


def exact_crop_reduce(frames, crop, size):
    """The patch by crop_area_cases.twin_patch, which slices, then exact_reduce."""
    return exact_reduce(cc.twin_patch(frames, *crop), *size)


# -- the sides' limit -------------------------------------------------------------------------------
LIMITS = ('widest', 'tallest')                                      # gif_cases' 65535 x 2 and 2 x 65535 (W x H)


def limit_frame(name):
    """[1, H, W, 3]"""
    return gc.case_frames(name, 1)


def _turned(name, pairs):
    return [p if name == 'widest' else p[::-1] for p in pairs]


def area_limit_targets(name):
    """(w, h): the copy, one pixel less along the long side (every target straddles two sources), just over half, a ratio that is no integer,
    one pixel."""
    return _turned(name, [(65535, 2), (65534, 2), (32768, 1), (40000, 2), (1, 1)])


def crop_limit_cases(name):
    """[(crop, size)]: crops that start on a half pixel along the long side, on whole pixels on both (the staged raw rows are the patch) and that
    are the frame's own sides (the last taps repeat the border pixel), each to the patch itself, to just over half of it and to one pixel."""
    out = []
    for cw, ch in ((65535 - 4, 1), (65535 - 5, 1), (65535, 2)):
        out += [((cw, ch), size) for size in ((cw, ch), (cw // 2 + 1, ch // 2 + 1), (1, 1))]
    return [(_turned(name, [crop])[0], _turned(name, [size])[0]) for crop, size in out]


def limit_depth(name):
    """dof_cases.depths at the frame's shape, one plane."""
    _, H, W, _ = limit_frame(name).shape
    return dc.depths(W, H, 1)


@functools.lru_cache(maxsize=None)
def limit_blur(name):
    """The header's blur of the limit frame at R = 16: the device's expected bytes there (a fifth of the twin's time; the two are held equal
    on the frame's ends in tests/test_filter_sweeps.py)."""
    want = dc.header_blur(limit_frame(name), limit_depth(name), dc.focus_of(1), dc.APERTURE, 16)
    want.setflags(write=False)
    return want


# -- the radius, made visible -------------------------------------------------------------------------
# A black frame two tiles each way whose background has radius 0, and white marks in front of it, 46 apart: each spreads over the background
# by exactly its own radius, so the output shows the radius the device computed.  A mark is a block of 3 x 3 pixels at one depth and not a
# single pixel: a lone sample of radius e reaches a background pixel with kWeight[e] of 8192 + kWeight[e], and from e = 13 on (weights 15, 13,
# 11, 10) 255 times that rounds to 0 -- the radii 13 .. 16 would all leave the same bytes.  At the rim of a block's reach up to four of its
# pixels add up, and predicted() below, a closed form for such frames, shows that every radius 0 .. 16 leaves bytes of its own.  The marks lie
# across the tiles' borders (columns 63 | 64, rows 15 | 16): their pixels and discs lie in neighbouring tiles, which know them only as
# staged halo cells.
MARK_W, MARK_H = 2 * TILE_X, 2 * TILE_Y['dof']
LAYOUTS = (((63, 15), (109, 16), (17, 15)), ((64, 16), (110, 15), (18, 16)))
BLOCK = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
f32 = np.float32
INF = f32(np.inf)
SMALLEST_NORMAL = f32(1.1754944e-38)


def _ties():
    cases = {}
    at, up, down = f32(64.0), np.nextafter(f32(64.0), INF), np.nextafter(f32(64.0), f32(0.0))
    for j in range(1, 17):
        A = f32(2 * j - 1)
        # A |64 - 96| = (j - 0.5) 64 exactly: the tie counts.  One ulp nearer the focus the left side shrinks and the right one grows: j - 1;
        # one ulp further from it both move the other way: still j.  With A one ulp smaller the tie itself is lost
        cases['tie j=%d' % j] = (96.0, A, f32(96.0), (at, up, down), (j, j - 1, j))
        cases['below the tie j=%d' % j] = (96.0, np.nextafter(A, f32(0.0)), f32(96.0), (at, up, down), (j - 1, None, None))
    return cases


# name -> (zf, A, the background's depth, the marks' depths, their radii at R = 16 as worked out by hand (None: whatever the twin gives))
RADIUS_CASES = _ties()
RADIUS_CASES.update({
    # products that overflow to +inf still compare; the background, behind everything and not finite, has radius 0
    'large A=20': (120.0, f32(20.0), INF, (f32(3e38), f32(1e-30), f32(60.0)), (16, 16, 16)),
    'large A=1e38': (120.0, f32(1e38), INF, (f32(3e38), f32(1e-30), f32(60.0)), (16, 16, 16)),
    # subnormal depths and a subnormal focus: valid (z > 0, finite), and every operation on them still one IEEE rounding
    'subnormal A=3': (1e-40, f32(3.0), INF, (f32(3e-40), f32(1.5e-40), f32(2.5e-40)), (2, 1, 2)),
    'subnormal A=1': (1e-40, f32(1.0), INF, (f32(3e-40), f32(1.5e-40), f32(2.5e-40)), (1, 0, 1)),
    'smallest normal A=3': (1e-40, f32(3.0), INF, (SMALLEST_NORMAL, f32(2.5e-40), f32(3e-40)), (3, 2, 2)),
    'smallest normal A=1': (1e-40, f32(1.0), INF, (SMALLEST_NORMAL, f32(2.5e-40), f32(3e-40)), (1, 1, 1))})
RADIUS_ORDER = list(RADIUS_CASES)


def mark_places(name):
    """(x, y) of the centres of the case's three marks: the layouts take turns and the marks move round a layout's places from case to case."""
    i = RADIUS_ORDER.index(name)
    layout = LAYOUTS[i // 2 % 2]
    return [layout[(k + i // 2) % 3] for k in range(3)]


def marked_frame(name):
    """-> (frame [1, H, W, 3], depth [1, H, W], the marks' centres (x, y))"""
    zf, A, background, marks, _ = RADIUS_CASES[name]
    frame, depth = np.zeros((1, MARK_H, MARK_W, 3), np.uint8), np.full((1, MARK_H, MARK_W), background, np.float32)
    places = mark_places(name)
    for (x, y), z in zip(places, marks):
        frame[0, y - 1:y + 2, x - 1:x + 2], depth[0, y - 1:y + 2, x - 1:x + 2] = 255, z
    return frame, depth, places


def predicted(places, radii):
    """[H, W]: every channel of the blurred marked frame, in closed form.  A background pixel has radius 0 and the weight 8192, and the only other
    samples that reach it are the c pixels of a mark of radius r that lie within r of it, white, kWeight[r] each; a mark's own pixels are reached
    by nothing but white."""
    y, x = np.mgrid[0:MARK_H, 0:MARK_W]
    white = np.zeros((MARK_H, MARK_W), np.int64)
    for (mx, my), r in zip(places, radii):
        white += dc.WEIGHT[r] * sum(((x - mx - dx) ** 2 + (y - my - dy) ** 2 <= r * r).astype(np.int64) for dx, dy in BLOCK)
    out = (2 * 255 * white + 8192 + white) // (2 * (8192 + white))
    for mx, my in places:
        out[my - 1:my + 2, mx - 1:mx + 2] = 255
    return out


@functools.lru_cache(maxsize=None)
def radius_case(name):
    """The twin and the header give the marks the radii the case is about, and the background 0; the twin's bytes are predicted()'s; and a
    mark whose radius were one more or one less would leave other bytes.  -> (frame, depth, the twin's bytes)"""
    zf, A, background, marks, stated = RADIUS_CASES[name]
    frame, depth, places = marked_frame(name)
    radii = dc.twin_radius(np.array(marks, np.float32), zf, A, 16).tolist()
    for of in (dc.twin_radius, dc.header_radius):
        assert of(np.array(marks, np.float32), zf, A, 16).tolist() == radii and of(np.array([background], np.float32), zf, A, 16).tolist() == [0], (name, of.__name__)
    assert all(want is None or want == got for want, got in zip(stated, radii)), (name, radii)
    assert all(z <= background for z in marks)                                        # in front of the background, or level with it: e = r(mark)
    want = dc.twin_blur(frame, depth, [zf], A, 16)
    assert (want == predicted(places, radii)[None, :, :, None]).all(), name
    for k, r in enumerate(radii):
        for other in (r - 1, r + 1):
            if 0 <= other <= 16:
                assert not np.array_equal(predicted(places, radii[:k] + [other] + radii[k + 1:]), want[0, :, :, 0]), (name, k, other)
    want.setflags(write=False)
    return frame, depth, want
