// kbe_dof_block.h -- the project's ONE definition of kbe_dof_u8 (include/kbe_dof.h): a lens blur of a raw frame by the depth of every one of
// its pixels, as a gather.  Two compilations read it: hipcc into the kernel of kbe_dof.hip, and g++ into tests/dof_check.cpp, which runs it
// serially against a restatement that scatters.
//
// A raw W x H frame of 3-byte pixels, a plane z of W x H fp32 depths (the cloud's depth attribute, as render_f32[3] holds it), a focus depth
// zf (fp32, finite, > 0), an aperture A (fp32, finite, >= 0: the blur radius in raw-frame pixels of a point at infinity) and a cap R,
// 0 <= R <= kMaxRadius.  The output is a W x H frame; channels are treated alike and not swapped.
//
// (1) The radius of a pixel, an integer 0..R, with no division:
//       t = |z - zf|                     one fp32 subtraction and its absolute value
//       lhs = A * t                      one fp32 multiplication
//       r = the number of j in 1..R with lhs >= (j - 0.5) * z      (one fp32 multiplication each; j - 0.5 is exact)
//     which is min(R, round(A |z - zf| / z)) stated so that every operation is a single IEEE rounding and none a multiply-add a compiler
//     could contract (-ffp-contract=off is part of the build all the same).  A depth that is not finite or not > 0 -- a hole nothing could
//     fill, NaN, +-inf, 0, a negative value -- gives r = 0.  A subnormal z or zf is a depth like any other (z > 0, finite): the operations
//     above keep their one rounding in the subnormal range, so neither compilation may flush fp32 denormals to zero (no -ffast-math, no
//     -fgpu-flush-denormals-to-zero; hipcc's default for gfx9 keeps them).  zf = 1e-40, A = 3: z = 3e-40, 1.5e-40, 2.5e-40 give 2, 1, 2.
// (2) The gather.  For a target pixel p and every sample pixel q INSIDE the frame with |dx|, |dy| <= R (no border is repeated):
//       e = r(q)                 when z(q) <= z(p), a plain fp32 comparison: a sample in front of the target, or level with it;
//       e = min(r(q), r(p))      otherwise: a sample behind the target never spreads further over it than the target is blurred itself;
//       q contributes iff dx^2 + dy^2 <= e^2, with the weight kWeight[e] = 8192 / n(e) in integer division, n(e) the number of lattice
//       points in the closed disc of radius e.  p always contributes to itself (d = 0) with kWeight[r(p)].
// (3) Per channel out = (2 sum(w v) + sum(w)) / (2 sum(w)) in integer division: the weighted mean, rounded half up.
//     Every sum fits 32 bits: a sample at d > 0 has e >= 1, a weight of at most kWeight[1] = 1638, and there are at most 33 * 33 - 1 = 1088
//     of them, so sum(w v) <= 8192 * 255 + 1088 * 1638 * 255 = 456 535 680, twice that plus sum(w) <= 914 861 696 < 2^32
//     (tests/dof_check.cpp asserts it from the table).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_DOF_HD __host__ __device__ __forceinline__
#else
#define KBE_DOF_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "kbe_rows.h"

namespace kbe_dof {

using kbe_rows::kMaxSide;

constexpr int kMaxRadius = 16;
constexpr uint32_t kUnit = 8192u;                       // kWeight[0]: the weight of a pixel that is in focus

// n(e): the lattice points of the closed disc of radius e, by counting
constexpr uint32_t disc_points(int e)
{
    uint32_t n = 0;
    for (int dy = -e; dy <= e; dy++)
        for (int dx = -e; dx <= e; dx++) n += dx * dx + dy * dy <= e * e ? 1u : 0u;
    return n;
}

struct Weights {
    uint32_t w[kMaxRadius + 1];
};

constexpr Weights make_weights()
{
    Weights t = {};
    for (int e = 0; e <= kMaxRadius; e++) t.w[e] = kUnit / disc_points(e);
    return t;
}

constexpr Weights kWeight = make_weights();

KBE_DOF_HD bool shape_ok(int W, int H, int R)
{
    return W >= 1 && H >= 1 && W <= kMaxSide && H <= kMaxSide && R >= 0 && R <= kMaxRadius;
}

// (1)
KBE_DOF_HD uint32_t radius(float z, float zf, float A, int R)
{
    if (!(z > 0.0f && z <= 3.40282346638528859812e+38f)) return 0u;      // NaN, +-inf, 0 and negative depths
    const float t = __builtin_fabsf(z - zf);
    const float lhs = A * t;
    uint32_t r = 0u;
    for (int j = 1; j <= kMaxRadius; j++) {
        const float rhs = ((float) j - 0.5f) * z;
        r += j <= R && lhs >= rhs ? 1u : 0u;
    }
    return r;
}

// (2) how far sample q spreads over target p
KBE_DOF_HD uint32_t extent(uint32_t rq, float zq, uint32_t rp, float zp)
{
    return zq <= zp ? rq : (rq < rp ? rq : rp);
}

KBE_DOF_HD bool covers(int dx, int dy, uint32_t e)
{
    return (uint32_t) (dx * dx + dy * dy) <= e * e;
}

// the sums of a target pixel: sum(w) and sum(w v) per channel, 32 bits each
struct Sums {
    uint32_t w, v[3];
};

// one contribution of weight `weight` (kWeight.w[e], however the caller keeps that table) and colour (v0, v1, v2)
KBE_DOF_HD void add(Sums& s, uint32_t weight, uint32_t v0, uint32_t v1, uint32_t v2)
{
    s.w += weight;
    s.v[0] += weight * v0;
    s.v[1] += weight * v1;
    s.v[2] += weight * v2;
}

// (3)
KBE_DOF_HD uint32_t rounded(uint32_t wv, uint32_t w)
{
    return (2u * wv + w) / (2u * w);
}

// the definition, serially: one target pixel from a frame, its depth plane and the plane of its radii (radius() of every depth) in memory
inline void gather_pixel(uint32_t W, uint32_t H, const uint8_t* src, size_t stride, const float* z, size_t z_stride, const uint8_t* r, int R, uint32_t x, uint32_t y, uint8_t out[3])
{
    const Weights table = kWeight;
    const uint32_t rp = r[(size_t) y * W + x];
    const float zp = z[(size_t) y * z_stride + x];
    const uint8_t* own = src + (size_t) y * stride + 3u * (size_t) x;
    Sums s = {0u, {0u, 0u, 0u}};
    add(s, table.w[rp], own[0], own[1], own[2]);
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++) {
            const long qx = (long) x + dx, qy = (long) y + dy;
            if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= (long) W || qy >= (long) H) continue;
            const uint32_t e = extent(r[(size_t) qy * W + qx], z[(size_t) qy * z_stride + qx], rp, zp);
            if (!covers(dx, dy, e)) continue;
            const uint8_t* q = src + (size_t) qy * stride + 3u * (size_t) qx;
            add(s, table.w[e], q[0], q[1], q[2]);
        }
    for (int c = 0; c < 3; c++) out[c] = (uint8_t) rounded(s.v[c], s.w);
}

}  // namespace kbe_dof
