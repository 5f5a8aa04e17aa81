// kbe_grade_block.h -- the project's ONE definition of the colour grade of kbe_grade_u8 (include/kbe_grade.h).  Two compilations read it:
// hipcc into the kernel of kbe_grade.hip, and g++ into tests/grade_check.cpp, which holds the packed forms below to the plain ones on all
// 2^24 colours and runs the rows serially.  The device's bytes are what grade_row below gives (tests/test_grade_gpu.py, through the NumPy twin).
//
// A 3D lookup table with tetrahedral interpolation over 3-byte pixels, in place.  No floating point.
//
// The table has N nodes per axis, 2 <= N <= 33: N^3 dwords, entry (i2 * N + i1) * N + i0 the node at frame byte 0 = i0, byte 1 = i1,
// byte 2 = i2; its bytes 0..2 are the output's bytes 0..2, byte 3 is ignored.  Nothing here knows of R, G or B.
//
// Cell and fraction of a byte v:   p = v (N - 1),  i = p / 255,  f = p - 255 i;  where i == N - 1 (only v = 255): i = N - 2, f = 255.
// So 0 <= i <= N - 2 and 0 <= f <= 255.
//
// With the three fractions ordered f_a >= f_b >= f_c (axes a, b, c) the four nodes are V0 = the cell's base node, V1 = V0 + e_a,
// V2 = V1 + e_b, V3 = the cell's far corner, and per output byte
//     g   = (V0 (255 - f_a) + V1 (f_a - f_b) + V2 (f_b - f_c) + V3 f_c + 127) / 255         (integer division; the weights add up to 255, so
//                                                                                            the numerator is at most 255 * 255 + 127 = 65152)
//     out = (c (256 - s) + g s + 128) >> 8                                                   (the strength s in 0..256; at most 65408)
// s = 256 gives g, s = 0 gives c.
//
// A tie does not matter: with f_a == f_b the node V1, the only one that depends on which of the two axes comes first, has the weight
// f_a - f_b = 0, and with f_b == f_c the same holds of V2.  So the bytes do not depend on how a sort breaks a tie (grade_check brute: all six
// orders of looking at the axes, on every colour).
//
// What follows from the definition:
//   * an identity table whose nodes are 255 j / (N - 1) EXACTLY -- the N with (N - 1) | 255: 2, 4, 6, 16, 18 -- leaves every colour as it
//     is: channel k of the four nodes is T(i_k) or T(i_k + 1), the weights of those with T(i_k + 1) add up to f_k whatever the order, so
//     255 g = 255 T(i_k) + (T(i_k + 1) - T(i_k)) f_k + 127 = 255 v + 127;
//   * for any N the result lies within 1 count of the same interpolation of unrounded nodes, rounded to nearest: a node's rounding is at
//     most 0.5, the convex combination keeps that, and the final rounding adds at most 0.5 on each side.
//
// The packed forms, which the kernel uses instead of the plain ones (and which are the plain ones: grade_check brute):
//   * the divisions by 255: with m = n + 1, n / 255 = (m + (m >> 8)) >> 8 for every n <= 65152 (csrc/kbe_overlay_block.h has the reason), which
//     two 16-bit lanes take side by side, and n / 255 = (n * 32897) >> 23 for every n < 65536, one multiply, where a value stands alone;
//   * the cell needs no comparison: i = min(p, 255 (N - 1) - 1) / 255, f = p - 255 i;
//   * bytes 0 and 2 of a node are weighted in the two 16-bit lanes of one dword, byte 1 beside them: no lane exceeds 65408, so nothing is
//     carried from one to the other;
//   * every product is the chip's 24-bit multiply (mul24), which runs at four times the rate of a 32-bit one;
//   * the fractions are ordered by minima and maxima, and three comparisons name the axis of the largest and the axis of the least;
//   * a lane of the kernel owns a RUN of 16 whole pixels, 48 bytes = 12 dwords (unpack_run, pack_run: nothing is indexed by a variable);
//     where the run does not begin on a dword, its 12 dwords are cut out of the 13 aligned ones that hold them and put back the same way
//     (run_from_aligned, run_to_aligned: funnel shifts by bytes).
#pragma once
#include "kbe_shutter_block.h"

#define KBE_GRADE_HD KBE_SHUTTER_HD
#if defined(__HIPCC__)
#define KBE_GRADE_UNROLL _Pragma("unroll")      // a run's pixels side by side: their table reads are in flight together, and nothing is indexed by a variable
#else
#define KBE_GRADE_UNROLL
#endif

namespace kbe_grade {

using kbe_rows::align_bytes;
using kbe_rows::kMaxSide;

constexpr int kMinNodes = 2;
constexpr int kMaxNodes = 33;
constexpr int kMaxStrength = 256;
constexpr int kRunPixels = 16;                // the whole pixels one lane of the kernel owns: it alone reads and writes their bytes
constexpr int kRunBytes = 3 * kRunPixels;     // 48
constexpr int kRunDwords = kRunBytes / 4;     // 12
constexpr uint32_t kLanes02 = 0x00FF00FFu;    // bytes 0 and 2 of a dword, as two 16-bit lanes

// -- the plain forms ---------------------------------------------------------------------------
KBE_GRADE_HD void cell_plain(uint32_t v, uint32_t N, uint32_t* i, uint32_t* f)
{
    const uint32_t p = v * (N - 1u);
    *i = p / 255u;
    *f = p - 255u * *i;
    if (*i == N - 1u) *i = N - 2u, *f = 255u;
}

KBE_GRADE_HD uint32_t tetra_plain(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t fa, uint32_t fb, uint32_t fc)
{
    return (v0 * (255u - fa) + v1 * (fa - fb) + v2 * (fb - fc) + v3 * fc + 127u) / 255u;
}

KBE_GRADE_HD uint32_t mix_plain(uint32_t c, uint32_t g, uint32_t s)
{
    return (c * (256u - s) + g * s + 128u) >> 8;
}

// -- the packed forms --------------------------------------------------------------------------
// The chip's 24-bit multiply, one full-rate instruction where a 32-bit multiply takes four times as long: the low 32 bits of the product
// of the factors' low 24 bits.  Both factors are below 2^24 wherever it is used here -- bytes, fractions, weights, strengths, node indices and
// steps up to 33^2, and the two 16-bit lanes 0x00FF00FF --, and every product fits 32 bits.
KBE_GRADE_HD uint32_t mul24(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return (a & 0xFFFFFFu) * (b & 0xFFFFFFu);
#endif
}

// p - 255 q for q < 2^23, p >= 255 q: the signed 24-bit multiply-add, one full-rate instruction
KBE_GRADE_HD uint32_t less_255_times(uint32_t p, uint32_t q)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t) (__mul24((int) q, -255) + (int) p);
#else
    return p - 255u * q;
#endif
}

KBE_GRADE_HD uint32_t least(uint32_t a, uint32_t b)
{
    return a < b ? a : b;
}

KBE_GRADE_HD uint32_t most(uint32_t a, uint32_t b)
{
    return a > b ? a : b;
}

// n / 255 from m = n + 1, for n <= 65152: two 16-bit lanes of a dword can be divided side by side this way
KBE_GRADE_HD uint32_t div255(uint32_t m)
{
    return (m + (m >> 8)) >> 8;
}

// n / 255 for n < 65536 by one 24-bit multiply: floor(n * 32897 / 2^23) (32897 / 2^23 is (1 + 1.5e-5) / 255: the excess stays below 1 / 255
// for these n, and n * 32897 < 2^32; grade_check forms tries every one)
KBE_GRADE_HD uint32_t div255_mul(uint32_t n)
{
    return mul24(n, 0x8081u) >> 23;
}

// The cell without a comparison: the least of p and 255 (N - 1) - 1 is p for every byte but 255, whose cell it makes N - 2; the fraction is
// taken from p itself, so that byte 255's is 255 (N - 1) - 255 (N - 2) = 255.
KBE_GRADE_HD void cell(uint32_t v, uint32_t N, uint32_t* i, uint32_t* f)
{
    const uint32_t p = mul24(v, N - 1u), q = div255_mul(least(p, mul24(255u, N - 1u) - 1u));
    *i = q;
    *f = less_255_times(p, q);
}

// the graded pixel g of the pixel x (bytes 0..2; byte 3 is not looked at) by a table of N nodes per axis: bytes 0..2, byte 3 = 0.
// The fractions are ordered by minima and maxima; of the axes only two are asked for, one whose fraction is the largest (its step: sa) and
// ANOTHER whose fraction is the least (sc) -- V1 = V0 + sa, and V2 = V3 - sc, the far corner less the last step.  With equal fractions the
// three comparisons still name two different axes, and which they name does not matter (above).
KBE_GRADE_HD uint32_t grade_pixel(uint32_t x, const uint32_t* lut, uint32_t N)
{
    uint32_t i0, i1, i2, f0, f1, f2;
    cell(x & 255u, N, &i0, &f0);
    cell((x >> 8) & 255u, N, &i1, &f1);
    cell((x >> 16) & 255u, N, &i2, &f2);
    const uint32_t NN = mul24(N, N), base = mul24(mul24(i2, N) + i1, N) + i0, far = base + 1u + N + NN;
    const uint32_t hi = most(f0, f1), lo = least(f0, f1), fa = most(hi, f2), fc = least(lo, f2), fb = least(hi, most(lo, f2));
    const bool g01 = f0 >= f1, g02 = f0 >= f2, g12 = f1 >= f2;
    const uint32_t sa = g01 && g02 ? 1u : g12 ? N : NN, sc = g12 && g02 ? NN : g01 ? N : 1u;
    const uint32_t v0 = lut[base], v1 = lut[base + sa], v2 = lut[far - sc], v3 = lut[far];
    const uint32_t w0 = 255u - fa, w1 = fa - fb, w2 = fb - fc, w3 = fc;
    const uint32_t even = mul24(v0 & kLanes02, w0) + mul24(v1 & kLanes02, w1) + mul24(v2 & kLanes02, w2) + mul24(v3 & kLanes02, w3) + 0x00800080u;
    const uint32_t odd = mul24((v0 >> 8) & 255u, w0) + mul24((v1 >> 8) & 255u, w1) + mul24((v2 >> 8) & 255u, w2) + mul24((v3 >> 8) & 255u, w3) + 128u;
    return (((even + ((even >> 8) & kLanes02)) >> 8) & kLanes02) | (div255(odd) << 8);
}

// mix_plain on bytes 0..2 of c and g
KBE_GRADE_HD uint32_t mix_pixel(uint32_t c, uint32_t g, uint32_t s)
{
    const uint32_t keep = (256u - s) & 0x1FFu, take = s & 0x1FFu;             // (0..256: said with a mask, so that the compiler sees factors of 24 bits)
    const uint32_t even = mul24(c & kLanes02, keep) + mul24(g & kLanes02, take) + 0x00800080u;
    const uint32_t odd = mul24((c >> 8) & 255u, keep) + mul24((g >> 8) & 255u, take) + 128u;
    return ((even >> 8) & kLanes02) | (odd & 0xFF00u);
}

// the 16 pixels of a run's 12 dwords, pixel k in bytes 0..2 of px[k] ...
KBE_GRADE_HD void unpack_run(const uint32_t c[kRunDwords], uint32_t px[kRunPixels])
{
    KBE_GRADE_UNROLL
    for (int q = 0; q < 4; q++) {
        const uint32_t d0 = c[3 * q], d1 = c[3 * q + 1], d2 = c[3 * q + 2];
        px[4 * q] = d0 & 0xFFFFFFu;
        px[4 * q + 1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
        px[4 * q + 2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
        px[4 * q + 3] = d2 >> 8;
    }
}

// ... and back (byte 3 of every px[k] is 0)
KBE_GRADE_HD void pack_run(const uint32_t px[kRunPixels], uint32_t c[kRunDwords])
{
    KBE_GRADE_UNROLL
    for (int q = 0; q < 4; q++) {
        const uint32_t p0 = px[4 * q], p1 = px[4 * q + 1], p2 = px[4 * q + 2], p3 = px[4 * q + 3];
        c[3 * q] = p0 | (p1 << 24);
        c[3 * q + 1] = (p1 >> 8) | (p2 << 16);
        c[3 * q + 2] = (p2 >> 16) | (p3 << 8);
    }
}

// a run in place: its 12 dwords graded at the strength s in 1..256 (a pixel beyond the run's own: whatever is there, graded as well)
KBE_GRADE_HD void grade_run(uint32_t c[kRunDwords], const uint32_t* lut, uint32_t N, uint32_t s)
{
    uint32_t px[kRunPixels];
    unpack_run(c, px);
    if (s == (uint32_t) kMaxStrength) {                                       // (mix_pixel(c, g, 256) is g: one frame's pixels all go one way)
        KBE_GRADE_UNROLL
        for (int k = 0; k < kRunPixels; k++) px[k] = grade_pixel(px[k], lut, N);
    } else {
        KBE_GRADE_UNROLL
        for (int k = 0; k < kRunPixels; k++) px[k] = mix_pixel(px[k], grade_pixel(px[k], lut, N), s);
    }
    pack_run(px, c);
}

// A run that begins b = 1..3 bytes into an aligned dword lies in 13 aligned dwords x[0..12], its bytes the bytes [b, b + 48) of them.
KBE_GRADE_HD void run_from_aligned(const uint32_t (&x)[kRunDwords + 1], uint32_t b, uint32_t (&c)[kRunDwords])
{
    kbe_rows::realign<kRunDwords>(x, b, c);
}

// ... and back: the bytes of x[0] before the run and of x[12] behind it are 0
KBE_GRADE_HD void run_to_aligned(const uint32_t c[kRunDwords], uint32_t b, uint32_t x[kRunDwords + 1])
{
    x[0] = align_bytes(c[0], 0u, 4u - b);
    for (int k = 1; k < kRunDwords; k++) x[k] = align_bytes(c[k], c[k - 1], 4u - b);
    x[kRunDwords] = align_bytes(0u, c[kRunDwords - 1], 4u - b);
}

#if !defined(__HIPCC__)
// The plain form of a whole pixel, the axes looked at in the order `order` = 0..5 (one of the six) and sorted stably from there: with equal
// fractions every order picks other nodes, and the bytes are the same.
inline uint32_t grade_plain(uint32_t x, const uint32_t* lut, uint32_t N, int order)
{
    static const int kOrders[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    uint32_t i[3], f[3];
    for (int k = 0; k < 3; k++) cell_plain((x >> (8 * k)) & 255u, N, &i[k], &f[k]);
    int axis[3] = {kOrders[order][0], kOrders[order][1], kOrders[order][2]};
    for (int a = 1; a < 3; a++)
        for (int b = a; b > 0 && f[axis[b]] > f[axis[b - 1]]; b--) {
            const int t = axis[b];
            axis[b] = axis[b - 1], axis[b - 1] = t;
        }
    const uint32_t step[3] = {1u, N, N * N}, base = (i[2] * N + i[1]) * N + i[0];
    const uint32_t v0 = lut[base], v1 = lut[base + step[axis[0]]], v2 = lut[base + step[axis[0]] + step[axis[1]]], v3 = lut[base + 1u + N + N * N];
    uint32_t out = 0u;
    for (int k = 0; k < 3; k++)
        out |= tetra_plain((v0 >> (8 * k)) & 255u, (v1 >> (8 * k)) & 255u, (v2 >> (8 * k)) & 255u, (v3 >> (8 * k)) & 255u, f[axis[0]], f[axis[1]], f[axis[2]]) << (8 * k);
    return out;
}

// One row of a frame on a CPU, serially and in place, the way the kernel takes it: runs of 16 pixels from the row's first byte; a whole run
// as 12 dwords -- through the 13 aligned ones around it where the row's address is no multiple of 4 (`lead`: that address, any number
// congruent to it modulo 4, given by the caller so that a test can walk through all four) --, the pixels of a row's last, shorter run byte
// by byte.  Nothing outside the row is read or written.
inline void grade_row(uint8_t* row, int32_t pixels, const uint32_t* lut, uint32_t N, uint32_t s, uint32_t lead)
{
    const uint32_t b = lead & 3u;
    for (int32_t first = 0; first < pixels; first += kRunPixels) {
        uint8_t* const p = row + 3l * first;
        const int32_t count = pixels - first < kRunPixels ? pixels - first : kRunPixels;
        uint32_t c[kRunDwords] = {0};
        if (count == kRunPixels && b != 0u) {
            uint8_t bytes[4 * (kRunDwords + 1)] = {0};
            uint32_t x[kRunDwords + 1];
            memcpy(bytes + b, p, kRunBytes);
            memcpy(x, bytes, sizeof(bytes));
            run_from_aligned(x, b, c);
            grade_run(c, lut, N, s);
            run_to_aligned(c, b, x);
            memcpy(bytes, x, sizeof(bytes));
            memcpy(p, bytes + b, kRunBytes);
        } else {
            memcpy(c, p, 3 * (size_t) count);
            grade_run(c, lut, N, s);
            memcpy(p, c, 3 * (size_t) count);
        }
    }
}
#endif

}  // namespace kbe_grade
