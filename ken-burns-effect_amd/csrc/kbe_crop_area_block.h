// kbe_crop_area_block.h -- the project's ONE definition of kbe_crop_area_u8 (include/kbe_crop_area.h): the centred crop of a raw frame, as
// crop_resize_body of kbe_hip.hip builds it in its step (1), reduced by the exact area average of kbe_area_block.h.  Two compilations read
// it: hipcc into the kernel of kbe_crop_area.hip, and g++ into tests/crop_area_check.cpp, which runs it serially against a brute-force
// restatement.  kbe_area_block.h is included as it is.
//
// A raw W x H frame of 3-byte pixels, a centred crop cw x ch (1 <= cw <= W, 1 <= ch <= H) and a target w x h (1 <= w <= cw, 1 <= h <= ch),
// all integers, no floating point anywhere.  The output is the area reduction with Shape{cw, ch, w, h} of the PATCH, the cw x ch image
// that cv2.getRectSubPix takes from the frame's centre:
//   per axis (N the frame's side, n the crop's) the patch starts at c = N / 2 - (n - 1) / 2 of the frame, a whole number when N - n is
//   odd and a whole number and a half when it is even: ip = floor(c) = (N - n + 1) >> 1, the fraction 0 or 1/2.  Patch pixel p of that
//   axis reads raw ip + p, and with the fraction 1/2 also raw ip + p + 1; a tap beyond the frame repeats the border pixel (only n == N
//   reaches one: ip + n <= N - 1 otherwise).  A patch pixel is, per channel,
//       whole pixel on both axes:      the raw pixel a
//       half pixel on one axis:        (a + b + 1) >> 1          of the two raw neighbours along it
//       half pixel on both:            (a + b + c + d + 2) >> 2  of the 2 x 2 raw neighbours
//   which are exactly (sum of a_ij v_ij + 32768) >> 16 with the 16-bit weights 65536, 32768 and 16384 the kernel of kbe_hip.hip computes
//   for these fractions.  With a whole axis' second tap set to its first, all three are the last form: (4 a + 2) >> 2 == a and
//   (2 a + 2 b + 2) >> 2 == (a + b + 1) >> 1; patch_value below is written that way.
// Two roundings, in this order, are the definition: the patch rounds to a byte, then the area mean of patch bytes rounds half up.
#pragma once
#include "kbe_area_block.h"

namespace kbe_crop_area {

using kbe_area::Shape;
using kbe_area::Window;

// the frame and its centred crop
struct Crop {
    uint32_t W, H, cw, ch;
};

KBE_AREA_HD bool shape_ok(int W, int H, int cw, int ch, int w, int h)
{
    return W >= 1 && H >= 1 && W <= kbe_rows::kMaxSide && H <= kbe_rows::kMaxSide && cw >= 1 && ch >= 1 && cw <= W && ch <= H && w >= 1 && h >= 1 && w <= cw && h <= ch;
}

// floor(c) of an axis, and whether c lies half a pixel beyond it
KBE_AREA_HD uint32_t start(uint32_t N, uint32_t n)
{
    return (N - n + 1u) >> 1;
}

KBE_AREA_HD bool half(uint32_t N, uint32_t n)
{
    return ((N - n) & 1u) == 0u;
}

// a crop that starts on whole pixels on both axes: the patch IS the raw rectangle at (start(W, cw), start(H, ch))
KBE_AREA_HD bool whole(const Crop& k)
{
    return !half(k.W, k.cw) && !half(k.H, k.ch);
}

// the two raw taps of patch index p on an axis: ip + p, and its neighbour (the border repeated) or itself
KBE_AREA_HD uint32_t tap0(uint32_t N, uint32_t n, uint32_t p)
{
    return start(N, n) + p;
}

KBE_AREA_HD uint32_t tap1(uint32_t N, uint32_t n, uint32_t p)
{
    const uint32_t t = tap0(N, n, p) + (half(N, n) ? 1u : 0u);
    return t < N ? t : N - 1u;
}

KBE_AREA_HD uint32_t patch_value(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return (a + b + c + d + 2u) >> 2;
}

// the patch of a frame in memory, as a Source of kbe_area::accumulate: row(py)(px, c) is the patch's byte
struct Patch {
    const uint8_t* base;
    size_t stride;
    Crop k;
    struct Row {
        const uint8_t* r0;
        const uint8_t* r1;
        uint32_t W, cw;
        KBE_AREA_HD uint32_t operator()(uint32_t px, int c) const
        {
            const size_t x0 = 3u * (size_t) tap0(W, cw, px) + c, x1 = 3u * (size_t) tap1(W, cw, px) + c;
            return patch_value(r0[x0], r0[x1], r1[x0], r1[x1]);
        }
    };
    KBE_AREA_HD Row row(uint32_t py) const
    {
        return Row{base + (size_t) tap0(k.H, k.ch, py) * stride, base + (size_t) tap1(k.H, k.ch, py) * stride, k.W, k.cw};
    }
};

// the definition, serially: one target pixel from a raw frame in memory
KBE_AREA_HD void crop_reduce_pixel(const Crop& k, uint32_t w, uint32_t h, const uint8_t* src, size_t stride, uint32_t ox, uint32_t oy, uint8_t out[3])
{
    const Shape g = {k.cw, k.ch, w, h};
    uint64_t acc[3] = {0u, 0u, 0u};
    kbe_area::accumulate(g, ox, oy, kbe_area::footprint(g, ox, oy), Patch{src, stride, k}, acc);
    for (int c = 0; c < 3; c++) out[c] = kbe_area::rounded(acc[c], g);
}

}  // namespace kbe_crop_area
