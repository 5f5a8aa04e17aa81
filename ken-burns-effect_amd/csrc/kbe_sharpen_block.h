// kbe_sharpen_block.h -- the project's ONE definition of kbe_sharpen_u8 (include/kbe_sharpen.h): an unsharp mask on 3-byte pixels, a separable
// Gaussian blur in integers and the difference to it added back.  Two compilations read it: hipcc into the kernel of kbe_sharpen.hip, and
// g++ into tests/sharpen_check.cpp, which runs it serially against the formulas evaluated in __int128.
//
// One channel byte v(x, y) of a W x H frame, clamp repeating the border pixel on both axes; taps w[0..R], 1 <= R <= kMaxRadius, 16 bits
// each, w[0] + 2 sum(w[1..R]) == kOne = 32768; amount 1..1024, the gain in 1/256; threshold 0..255.  No floating point anywhere:
//     h16(x, y) = (sum_{k=-R..R} w[|k|] v(clamp(x + k), y)   + 64)    >> 7       0..65280: the row blur, 8.8 fixed point
//     b16(x, y) = (sum_{k=-R..R} w[|k|] h16(x, clamp(y + k)) + 16384) >> 15      the blur, 8.8
//     d         = 256 v(x, y) - b16(x, y)
//     out       = v(x, y)                                          if |d| < 256 threshold
//               = clamp(v + ((amount d + 32768) >> 16), 0, 255)    otherwise; >> is a floor for negative values too
// Every sum fits a signed 32 bits.  The row pass: its terms are not negative and add up to at most 255 * 32768 + 64 < 2^23.  The column
// pass: at most 65280 * 32768 + 16384 = 2139111424 < 2^31 = 2147483648.  The gain: |d| <= 65280, so |amount d| + 32768 <= 1024 * 65280 +
// 32768 < 2^27.  A pass adds w[0] v(0) + sum_k w[k] (v(-k) + v(k)): the same terms in another order, every partial sum within the bounds.
// Because the taps add up to exactly kOne, a constant frame comes out unchanged: h16 = 256 v, b16 = 256 v, d = 0 -- and so does a 1 x 1
// frame.  Channels are independent and are not swapped.
#pragma once
#include "kbe_area_block.h"

namespace kbe_sharpen {

constexpr int kMaxRadius = 24;
constexpr int kOne = 32768;
constexpr int kMaxAmount = 1024, kMaxThreshold = 255;

// the taps of a call, as the kernel's arguments carry them: w[k] for k <= radius, 0 beyond
struct Taps {
    uint32_t w[kMaxRadius + 1];
    int32_t radius;
};

KBE_AREA_HD bool taps_ok(const uint16_t* taps, int radius)
{
    if (!(radius >= 1 && radius <= kMaxRadius)) return false;
    uint32_t sum = taps[0];
    for (int k = 1; k <= radius; k++) sum += 2u * taps[k];
    return sum == (uint32_t) kOne;
}

KBE_AREA_HD bool shape_ok(int W, int H, int amount, int threshold)
{
    return W >= 1 && H >= 1 && W <= kbe_rows::kMaxSide && H <= kbe_rows::kMaxSide && amount >= 1 && amount <= kMaxAmount && threshold >= 0 && threshold <= kMaxThreshold;
}

KBE_AREA_HD uint32_t clamped(int32_t i, uint32_t n)
{
    return i < 0 ? 0u : i > (int32_t) n - 1 ? n - 1u : (uint32_t) i;
}

// sum_{k=-R..R} w[|k|] at(k): at(k) is the value k steps from the centre along the pass, the clamp is the caller's
template <class At>
KBE_AREA_HD int32_t weighted(const Taps& t, At at)
{
    int32_t s = (int32_t) t.w[0] * (int32_t) at(0);
    for (int k = 1; k <= kMaxRadius; k++) {
        if (k > t.radius) break;
        s += (int32_t) t.w[k] * ((int32_t) at(-k) + (int32_t) at(k));
    }
    return s;
}

// the pass along a row, from bytes: 0..65280
template <class At>
KBE_AREA_HD uint32_t row_pass(const Taps& t, At at)
{
    return (uint32_t) ((weighted(t, at) + 64) >> 7);
}

// the pass down a column, from row_pass' values: 0..65280
template <class At>
KBE_AREA_HD uint32_t column_pass(const Taps& t, At at)
{
    return (uint32_t) ((weighted(t, at) + 16384) >> 15);
}

// the byte from the source byte and the blur; the shift of a negative value is arithmetic: a floor
KBE_AREA_HD uint32_t sharpened(uint32_t v, uint32_t b16, int32_t amount, int32_t threshold)
{
    const int32_t d = 256 * (int32_t) v - (int32_t) b16;
    if ((d < 0 ? -d : d) < 256 * threshold) return v;
    const int32_t s = (int32_t) v + ((amount * d + 32768) >> 16);
    return (uint32_t) (s < 0 ? 0 : s > 255 ? 255 : s);
}

// the definition, serially: one pixel of a frame in memory
KBE_AREA_HD void sharpen_pixel(const Taps& t, int32_t amount, int32_t threshold, const uint8_t* src, size_t stride, uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint8_t out[3])
{
    for (int c = 0; c < 3; c++) {
        const uint32_t b16 = column_pass(t, [&](int j) {
            const uint8_t* const row = src + (size_t) clamped((int32_t) y + j, H) * stride;
            return row_pass(t, [&](int k) { return (uint32_t) row[3u * (size_t) clamped((int32_t) x + k, W) + c]; });
        });
        out[c] = (uint8_t) sharpened(src[(size_t) y * stride + 3u * (size_t) x + c], b16, amount, threshold);
    }
}

}  // namespace kbe_sharpen
