// kbe_enlarge_block.h -- the project's ONE definition of kbe_enlarge_u8 (include/kbe_enlarge.h): the centred crop of a raw frame, the patch
// of kbe_crop_area_block.h as it is, enlarged by a separable Catmull-Rom bicubic in integers.  Two compilations read it: hipcc into the
// kernel of kbe_enlarge.hip, and g++ into tests/enlarge_check.cpp, which runs it serially against coefficients computed as exact rationals.
//
// A raw W x H frame of 3-byte pixels, a centred crop cw x ch (1 <= cw <= W, 1 <= ch <= H) and a target w x h (cw <= w <= kMaxOut,
// ch <= h <= kMaxOut), all integers, no floating point anywhere.  The patch cw x ch -- start, half, tap0, tap1 and patch_value of
// kbe_crop_area_block.h: bytes, with a rounding of their own -- is resampled on half-pixel centres, first along the rows into bytes, then
// down the columns of those bytes.  Per axis, output index x of n_out from n_in:
//     D = 2 n_out,   p = (2 x + 1) n_in - n_out,   i = floor(p / D),   r = p - i D   (0 <= r < D: the position is i + r / D)
//     the taps are i - 1 .. i + 2, each clamped to 0 .. n_in - 1: the border pixel repeats
//     the Catmull-Rom weights (a = -1/2) at t = r / D, as numerators over 2 D^3:
//         n0 = -r^3 + 2 r^2 D - r D^2     n1 = 3 r^3 - 5 r^2 D + 2 D^3     n2 = -3 r^3 + 4 r^2 D + r D^2     n3 = r^3 - r^2 D
//     c_k = floor((n_k 16384 + D^3) / (2 D^3)) for k = 0, 2, 3 -- a true floor, also of a negative numerator --, c1 = 16384 - c0 - c2 - c3
//     a pass: clamp((c0 v0 + c1 v1 + c2 v2 + c3 v3 + 8192) >> 14, 0, 255), the shift arithmetic
// Three roundings, in this order, are the definition: the patch to a byte, the pass along the rows to a byte, the pass down the columns.
// At n_out == n_in r is 0 and the coefficients are (0, 16384, 0, 0): the crop's own size gives the patch itself.
#pragma once
#include "kbe_crop_area_block.h"

namespace kbe_enlarge {

using kbe_crop_area::Crop;

// The longest side of a target.  With n_out <= 16384: D <= 2^15 and r < D, so r^3, r^2 D, r D^2 and D^3 are at most 2^45.  A numerator is
// a sum of such terms whose positive factors add up to at most 5 (n1: 3 + 2, n2: 4 + 1) and whose negative ones to at most 5 (n1), so
// |n_k| <= 5 * 2^45 and |n_k| * 16384 + D^3 <= 5 * 2^45 * 2^14 + 2^45 < 2^63: every product and sum fits an int64.
// p = (2 x + 1) n_in - n_out lies in (-2^14, 2^29) and i D in (-2^16, 2^29): an int32 each.
constexpr int kMaxOut = 16384;
constexpr int kOneBits = 14, kOne = 1 << kOneBits;

KBE_AREA_HD bool shape_ok(int W, int H, int cw, int ch, int w, int h)
{
    return W >= 1 && H >= 1 && W <= kbe_rows::kMaxSide && H <= kbe_rows::kMaxSide && cw >= 1 && ch >= 1 && cw <= W && ch <= H && w >= cw && h >= ch && w <= kMaxOut && h <= kMaxOut;
}

// floor(a / b), b > 0
KBE_AREA_HD int64_t floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return a - q * b < 0 ? q - 1 : q;
}

// i of output index x, and r through *r
KBE_AREA_HD int32_t position(uint32_t n_in, uint32_t n_out, uint32_t x, uint32_t* r)
{
    const int32_t D = 2 * (int32_t) n_out, p = (2 * (int32_t) x + 1) * (int32_t) n_in - (int32_t) n_out;
    const int32_t q = p / D, i = p - q * D < 0 ? q - 1 : q;
    *r = (uint32_t) (p - i * D);
    return i;
}

KBE_AREA_HD uint32_t clamped(int32_t tap, uint32_t n_in)
{
    return tap < 0 ? 0u : tap > (int32_t) n_in - 1 ? n_in - 1u : (uint32_t) tap;
}

// the four coefficients and the four clamped taps of an output index
struct Taps {
    int32_t c[4];
    uint32_t t[4];
};

KBE_AREA_HD Taps taps(uint32_t n_in, uint32_t n_out, uint32_t x)
{
    Taps a;
    uint32_t r32;
    const int32_t i = position(n_in, n_out, x, &r32);
    const int64_t D = 2 * (int64_t) n_out, r = r32, D3 = D * D * D, r2D = r * r * D, r3 = r * r * r, rD2 = r * D * D;
    a.c[0] = (int32_t) floor_div((-r3 + 2 * r2D - rD2) * kOne + D3, 2 * D3);
    a.c[2] = (int32_t) floor_div((-3 * r3 + 4 * r2D + rD2) * kOne + D3, 2 * D3);
    a.c[3] = (int32_t) floor_div((r3 - r2D) * kOne + D3, 2 * D3);
    a.c[1] = kOne - a.c[0] - a.c[2] - a.c[3];
    for (int k = 0; k < 4; k++) a.t[k] = clamped(i - 1 + k, n_in);
    return a;
}

// a pass over four bytes: |c_k| < 2^15 and v_k <= 255, the sum stays below 2^25
KBE_AREA_HD uint32_t pass(const int32_t c[4], uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3)
{
    const int32_t s = (c[0] * (int32_t) v0 + c[1] * (int32_t) v1 + c[2] * (int32_t) v2 + c[3] * (int32_t) v3 + (kOne >> 1)) >> kOneBits;
    return (uint32_t) (s < 0 ? 0 : s > 255 ? 255 : s);
}

// the definition, serially: one target pixel from a raw frame in memory
KBE_AREA_HD void enlarge_pixel(const Crop& k, uint32_t w, uint32_t h, const uint8_t* src, size_t stride, uint32_t ox, uint32_t oy, uint8_t out[3])
{
    const Taps ax = taps(k.cw, w, ox), ay = taps(k.ch, h, oy);
    const kbe_crop_area::Patch patch = {src, stride, k};
    for (int c = 0; c < 3; c++) {
        uint32_t along[4];
        for (int j = 0; j < 4; j++) {
            const kbe_crop_area::Patch::Row row = patch.row(ay.t[j]);
            along[j] = pass(ax.c, row(ax.t[0], c), row(ax.t[1], c), row(ax.t[2], c), row(ax.t[3], c));
        }
        out[c] = (uint8_t) pass(ay.c, along[0], along[1], along[2], along[3]);
    }
}

}  // namespace kbe_enlarge
