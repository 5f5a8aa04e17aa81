// kbe_area_block.h -- the project's ONE definition of the exact area-average reduction of kbe_area_reduce_u8 (include/kbe_area.h).
// Two compilations read it: hipcc into the kernel of kbe_area.hip, and g++ into tests/area_check.cpp, which runs it serially against a
// brute-force restatement.  The device's bytes are what reduce_pixel below gives (tests/test_area_gpu.py, through the NumPy twin).
//
// A W x H source becomes a w x h target, 1 <= w <= W, 1 <= h <= H, all integers, no floating point anywhere.  Per axis (N source cells,
// n target cells) both lie on one axis of N * n units: source cell s covers [s n, (s + 1) n), target cell o covers [o N, (o + 1) N).
// weight(o, s, N, n) is the length of their overlap, 0..n: over the sources of one target the weights add up to N, over the targets of
// one source to n.  Per channel
//     S   = sum over sy, sx of  weight(oy, sy, H, h) * weight(ox, sx, W, w) * v[sy][sx]
//     out = (2 S + W H) / (2 W H)          (integer division: the mean, rounded half up)
// The sum over sx is taken first: at most 255 W, 32 bits for W <= 65535; the sum over sy takes 64.  Every product n * N stays below 2^32.
// w == W and h == H copies: every weight is N or 0.  Channels are not swapped.
//
// accumulate() adds the part of S that lies in a WINDOW of the source, so a kernel may take a footprint in pieces (strips staged in LDS):
// the sums are exact, the order of the pieces does not matter.  A window wider than the footprint adds nothing: weight is 0 outside it.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_AREA_HD __host__ __device__ __forceinline__
#else
#define KBE_AREA_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "kbe_rows.h"

namespace kbe_area {

using kbe_rows::kMaxSide;

struct Shape {
    uint32_t W, H, w, h;
};

// the sources [x0, x1) x [y0, y1) that a target pixel overlaps, or any window of the source
struct Window {
    uint32_t x0, x1, y0, y1;
};

KBE_AREA_HD bool shape_ok(int W, int H, int w, int h)
{
    return W >= 1 && H >= 1 && W <= kMaxSide && H <= kMaxSide && w >= 1 && h >= 1 && w <= W && h <= H;
}

// the first source cell that target cell o overlaps, and one past the last: floor(o N / n), ceil((o + 1) N / n)
KBE_AREA_HD uint32_t span_begin(uint32_t o, uint32_t N, uint32_t n)
{
    return o * N / n;
}

KBE_AREA_HD uint32_t span_end(uint32_t o, uint32_t N, uint32_t n)
{
    return ((o + 1u) * N + n - 1u) / n;
}

KBE_AREA_HD uint32_t weight(uint32_t o, uint32_t s, uint32_t N, uint32_t n)
{
    const uint32_t s0 = s * n, s1 = s0 + n, o0 = o * N, o1 = o0 + N;
    const uint32_t lo = s0 > o0 ? s0 : o0, hi = s1 < o1 ? s1 : o1;
    return hi > lo ? hi - lo : 0u;
}

KBE_AREA_HD Window footprint(const Shape& g, uint32_t ox, uint32_t oy)
{
    return Window{span_begin(ox, g.W, g.w), span_end(ox, g.W, g.w), span_begin(oy, g.H, g.h), span_end(oy, g.H, g.h)};
}

KBE_AREA_HD Window intersect(const Window& a, const Window& b)
{
    return Window{a.x0 > b.x0 ? a.x0 : b.x0, a.x1 < b.x1 ? a.x1 : b.x1, a.y0 > b.y0 ? a.y0 : b.y0, a.y1 < b.y1 ? a.y1 : b.y1};
}

// acc[c] += the part of S of target pixel (ox, oy) that comes from the sources in `in`.  source.row(sy) gives that row, row(sx, c) its
// pixel sx's channel c, 0..255.
template <class Source>
KBE_AREA_HD void accumulate(const Shape& g, uint32_t ox, uint32_t oy, const Window& in, const Source& source, uint64_t acc[3])
{
    for (uint32_t sy = in.y0; sy < in.y1; sy++) {
        const uint32_t wy = weight(oy, sy, g.H, g.h);
        const auto row = source.row(sy);
        uint32_t along[3] = {0u, 0u, 0u};
        for (uint32_t sx = in.x0; sx < in.x1; sx++) {
            const uint32_t wx = weight(ox, sx, g.W, g.w);
            for (int c = 0; c < 3; c++) along[c] += wx * row(sx, c);
        }
        for (int c = 0; c < 3; c++) acc[c] += (uint64_t) wy * along[c];
    }
}

KBE_AREA_HD uint8_t rounded(uint64_t S, const Shape& g)
{
    const uint64_t area = (uint64_t) g.W * g.H;
    return (uint8_t) ((2u * S + area) / (2u * area));
}

// rows of 3-byte pixels in memory
struct Rows {
    const uint8_t* base;
    size_t stride;
    struct Row {
        const uint8_t* p;
        KBE_AREA_HD uint32_t operator()(uint32_t sx, int c) const { return p[3u * (size_t) sx + c]; }
    };
    KBE_AREA_HD Row row(uint32_t sy) const { return Row{base + (size_t) sy * stride}; }
};

// the definition, serially: one target pixel from a source in memory
KBE_AREA_HD void reduce_pixel(const Shape& g, const uint8_t* src, size_t stride, uint32_t ox, uint32_t oy, uint8_t out[3])
{
    uint64_t acc[3] = {0u, 0u, 0u};
    accumulate(g, ox, oy, footprint(g, ox, oy), Rows{src, stride}, acc);
    for (int c = 0; c < 3; c++) out[c] = rounded(acc[c], g);
}

}  // namespace kbe_area
