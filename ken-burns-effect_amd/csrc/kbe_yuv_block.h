// kbe_yuv_block.h -- the project's ONE definition of the 4:2:0 planes of kbe_yuv420_u8 (include/kbe_yuv.h).  Two compilations read it: hipcc
// into the kernel of kbe_yuv.hip, and g++ into tests/yuv_check.cpp, which holds the packed forms below to the plain one on every input they
// can meet and runs whole frames serially, lane by lane.  The device's bytes are what convert_frame below gives (tests/test_yuv_gpu.py,
// through the NumPy twin).
//
// The input is an H x W frame of 3-byte pixels; R, G, B are a pixel's bytes after the BGR flag has swapped the first and the third.  BT.601 at
// limited range, in integers:
//     Y  = 16 + ((66 R + 129 G + 25 B + 128) >> 8)                                      for every pixel, 16..235
//     Cb = 128 + floor((-38 Rs - 74 Gs + 112 Bs + 128 n) / (256 n))                     for every cell, 16..240
//     Cr = 128 + floor((112 Rs - 94 Gs - 18 Bs + 128 n) / (256 n))
// Chroma has cw x ch cells, cw = (W + 1) / 2, ch = (H + 1) / 2; cell (cx, cy) covers the pixels x in {2 cx, 2 cx + 1}, y in {2 cy, 2 cy + 1}
// that exist, n = 1, 2 or 4 of them, and Rs, Gs, Bs are their sums: the cell's centre is the chroma site (C420jpeg).  128 * 256 n is added
// before the shift by 8 + log2 n, so nothing negative is shifted (cb_of, cr_of).  A frame's payload is W H + 2 cw ch bytes: the Y plane (rows
// of W), the Cb plane (rows of cw), the Cr plane.  No floating point.
//
// The packed forms, which the kernel uses instead of the plain ones (and which are the plain ones: yuv_check brute):
//   * a pixel is taken as the DWORD that starts at its first byte, p = b0 | b1 << 8 | b2 << 16 | (the next pixel's first byte) << 24; a sum of
//     products is dot4(p, w, c) = c + the sum of the four byte products, the chip's v_dot4_u32_u8, with the weight of byte 3 always 0.
//   * luma: dot4(p, wy, 128 + 4096) holds Y in its byte 1 (at most 220 * 255 + 128 + 4096 = 60324).
//   * chroma: a negative weight -k on a byte v is k (255 - v) - 255 k, and 255 - v is v ^ 0xFF: the bytes with negative weights are flipped
//     by one XOR of the pixel (Coef::xcb, xcr), all weights are positive, and the constant is put into dot4's addend.  Both matrices' negative
//     weights add up to 112.
//   * a cell is always summed over FOUR pixel dwords: where the right column or the bottom row does not exist, the pixel beside it is taken
//     twice.  Doubling the sums and n leaves floor((sum + 128 n) / (256 n)) what it was, so n = 2 and n = 1 are the n = 4 form on repeated
//     pixels: cell = (17344 + the four dots) >> 10, 17344 = 512 + 128 * 1024 - 4 * 255 * 112, at most 245824 >> 10 = 240.
//   * a lane takes a RUN of kRun = 16 pixels, 8 cells, of a row pair: 48 source bytes of each row, which start anywhere; they are cut out of
//     the 13 ALIGNED dwords that hold them (csrc/kbe_rows.h's realign), and pixel i is cut out of those (pixel).
//   * the four output streams of a row pair -- the two Y rows, the Cb row, the Cr row -- start anywhere too, each at an alignment of its
//     own.  A lane's bytes of a stream are moved up by m = the stream's address modulo 4 with the previous lane's last dword (shift_in), so
//     that every lane stores ALIGNED dwords (store_piece); byte stores are left to a stream's two ends.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_YUV_HD __host__ __device__ __forceinline__
#else
#define KBE_YUV_HD inline
#endif
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "kbe_rows.h"

namespace kbe_yuv {

using kbe_rows::align_bytes;
using kbe_rows::kMaxSide;
using kbe_rows::realign;

constexpr int kFlagBGR = 1;                   // KBE_YUV_BGR
constexpr int kRun = 16;                      // pixels of a row that one lane of the kernel takes: 8 cells
constexpr int kRunDwords = 12;                // ... 48 source bytes of each of its two rows
constexpr int kCells = kRun / 2;
constexpr uint32_t kLumaAddend = 128u + 4096u;
constexpr uint32_t kChromaAddend = 512u + 128u * 1024u - 4u * 255u * 112u;      // 17344
static_assert(kChromaAddend == 17344u && 38 + 74 == 112 && 94 + 18 == 112, "the chroma constant");

// -- the plain forms -------------------------------------------------------------------------------------------------------------------
KBE_YUV_HD uint32_t luma_of(uint32_t R, uint32_t G, uint32_t B)
{
    return 16u + ((66u * R + 129u * G + 25u * B + 128u) >> 8);
}

// Rs, Gs, Bs: the sums over the n = 1 << log2n pixels of a cell
KBE_YUV_HD uint32_t cb_of(int Rs, int Gs, int Bs, int log2n)
{
    const int n = 1 << log2n;
    return (uint32_t) ((-38 * Rs - 74 * Gs + 112 * Bs + 128 * n + 128 * 256 * n) >> (8 + log2n));
}

KBE_YUV_HD uint32_t cr_of(int Rs, int Gs, int Bs, int log2n)
{
    const int n = 1 << log2n;
    return (uint32_t) ((112 * Rs - 94 * Gs - 18 * Bs + 128 * n + 128 * 256 * n) >> (8 + log2n));
}

KBE_YUV_HD size_t payload_bytes(long W, long H)
{
    return W >= 1 && W <= kMaxSide && H >= 1 && H <= kMaxSide ? (size_t) W * (size_t) H + 2u * (size_t) ((W + 1) / 2) * (size_t) ((H + 1) / 2) : (size_t) 0;
}

// -- the packed forms ------------------------------------------------------------------------------------------------------------------
// The weights of a pixel dword's bytes, and the bytes to flip, for the channel order of the flags
struct Coef {
    uint32_t wy, wcb, xcb, wcr, xcr;
};

KBE_YUV_HD Coef coef(int flags)
{
    Coef k;
    if (flags & kFlagBGR) {                   // byte 0 is B, byte 2 is R
        k.wy = 25u | 129u << 8 | 66u << 16;
        k.wcb = 112u | 74u << 8 | 38u << 16, k.xcb = 0x00FFFF00u;
        k.wcr = 18u | 94u << 8 | 112u << 16, k.xcr = 0x0000FFFFu;
    } else {
        k.wy = 66u | 129u << 8 | 25u << 16;
        k.wcb = 38u | 74u << 8 | 112u << 16, k.xcb = 0x0000FFFFu;
        k.wcr = 112u | 94u << 8 | 18u << 16, k.xcr = 0x00FFFF00u;
    }
    return k;
}

// c + a.b0 w.b0 + a.b1 w.b1 + a.b2 w.b2 + a.b3 w.b3.  On the device one instruction, by its builtin; the form below it is what that
// instruction computes, and what a CPU runs
KBE_YUV_HD uint32_t dot4(uint32_t a, uint32_t w, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, w, c, false);
#else
    for (int i = 0; i < 4; i++) c += ((a >> (8 * i)) & 0xFFu) * ((w >> (8 * i)) & 0xFFu);
    return c;
#endif
}

// byte 1 of a, b, c and d as the bytes 0, 1, 2 and 3 of one dword: on the device three byte permutes
KBE_YUV_HD uint32_t bytes1(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t ab = __builtin_amdgcn_perm(b, a, 0x0c0c0501u), cd = __builtin_amdgcn_perm(d, c, 0x0c0c0501u);
    return __builtin_amdgcn_perm(cd, ab, 0x05040100u);
#else
    return ((a >> 8) & 0xFFu) | (b & 0xFF00u) | ((c << 8) & 0xFF0000u) | ((d << 16) & 0xFF000000u);
#endif
}

// Y of the pixel dword p, in byte 1 of the result
KBE_YUV_HD uint32_t luma_word(uint32_t p, uint32_t wy)
{
    return dot4(p, wy, kLumaAddend);
}

// Cb or Cr of a cell from its four pixel dwords (a pixel that does not exist: the one beside it again), weights w, flipped bytes x
KBE_YUV_HD uint32_t chroma_of(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t w, uint32_t x)
{
    return dot4(p3 ^ x, w, dot4(p2 ^ x, w, dot4(p1 ^ x, w, dot4(p0 ^ x, w, kChromaAddend)))) >> 10;
}

// pixel i of a run, as a dword, from the run's 12 dwords; byte 3 of the last pixel's is 0.  i is a constant wherever this is called
KBE_YUV_HD uint32_t pixel(const uint32_t (&w)[kRunDwords], int i)
{
    const int k = (3 * i) >> 2, r = (3 * i) & 3;
    return r == 0 ? w[k] : align_bytes(k + 1 < kRunDwords ? w[k + 1] : 0u, w[k], (uint32_t) r);
}

// One lane's work: the 16 pixels of two rows -> their Y bytes (4 dwords a row), their 8 Cb and 8 Cr bytes (2 dwords each).  `lone`: the cell
// of the run whose right pixel does not exist (the last cell of a row of odd width), or -1.  Without a bottom row the caller passes the top
// row twice.  What lies beyond the row's last pixel gives bytes that nobody stores.
KBE_YUV_HD void run(const uint32_t (&top)[kRunDwords], const uint32_t (&bot)[kRunDwords], int lone, const Coef& k, uint32_t (&ytop)[4], uint32_t (&ybot)[4],
                    uint32_t (&cb)[2], uint32_t (&cr)[2])
{
    uint32_t yt[kRun], yb[kRun], u[kCells], v[kCells];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < kCells; c++) {
        const uint32_t tl = pixel(top, 2 * c), bl = pixel(bot, 2 * c);
        uint32_t tr = pixel(top, 2 * c + 1), br = pixel(bot, 2 * c + 1);
        yt[2 * c] = luma_word(tl, k.wy), yt[2 * c + 1] = luma_word(tr, k.wy);
        yb[2 * c] = luma_word(bl, k.wy), yb[2 * c + 1] = luma_word(br, k.wy);
        if (c == lone) tr = tl, br = bl;
        u[c] = chroma_of(tl, tr, bl, br, k.wcb, k.xcb);
        v[c] = chroma_of(tl, tr, bl, br, k.wcr, k.xcr);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < 4; q++) {
        ytop[q] = bytes1(yt[4 * q], yt[4 * q + 1], yt[4 * q + 2], yt[4 * q + 3]);
        ybot[q] = bytes1(yb[4 * q], yb[4 * q + 1], yb[4 * q + 2], yb[4 * q + 3]);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < 2; q++) {
        cb[q] = u[4 * q] | u[4 * q + 1] << 8 | u[4 * q + 2] << 16 | u[4 * q + 3] << 24;
        cr[q] = v[4 * q] | v[4 * q + 1] << 8 | v[4 * q + 2] << 16 | v[4 * q + 3] << 24;
    }
}

// (Which of the 13 ALIGNED dwords around a run's 48 source bytes hold a byte of the row, and so may be loaded: kbe_rows.h's
// dword_holds_a_byte<kRunDwords> and all_dwords_hold_a_byte<kRunDwords>, on the kernel's int.)

// A lane's N dwords of an output stream, moved up by m = the stream's address modulo 4 -> N + 1 dwords, out[0] beginning with the last m
// bytes of the previous lane's last dword `prev`; out[N] holds the lane's own last m bytes, which the stream's last lane stores itself
template <int N>
KBE_YUV_HD void shift_in(const uint32_t (&own)[N], uint32_t prev, uint32_t m, uint32_t (&out)[N + 1])
{
    if (m == 0u) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int d = 0; d < N; d++) out[d] = own[d];
        out[N] = 0u;
    } else {
        out[0] = align_bytes(own[0], prev, 4u - m);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int d = 1; d < N; d++) out[d] = align_bytes(own[d], own[d - 1], 4u - m);
        out[N] = align_bytes(0u, own[N - 1], 4u - m);
    }
}

// (what the device stores as one piece at the alignment of a dword)
struct __attribute__((packed, aligned(4))) Stored4 {
    uint32_t x, y, z, w;
};
struct __attribute__((packed, aligned(4))) Stored2 {
    uint32_t x, y;
};

KBE_YUV_HD void store_dword(uint8_t* p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint32_t*>(p) = v;             // p is a multiple of 4 there
#else
    memcpy(p, &v, 4);
#endif
}

// The first n of a lane's N + 1 shifted dwords to the stream `row` of nbytes bytes, the first of them at the byte `at` of the stream (at +
// the stream's address is a multiple of 4; at is -m for the first lane).  Dwords that lie inside the stream are stored as dwords, the lane's own N
// at once (16 or 8 bytes) where all of them do; of a dword across one of the stream's two ends, the bytes inside one by one; nothing else.
template <int N>
KBE_YUV_HD void store_piece(uint8_t* row, int nbytes, int at, const uint32_t (&w)[N + 1], int n)
{
    int d = 0;
    if (at >= 0 && at + 4 * N <= nbytes) {            // inside the stream: every lane but a stream's first and last
#if defined(__HIP_DEVICE_COMPILE__)
        if (N == 4) {
            Stored4 s;
            s.x = w[0], s.y = w[1], s.z = w[2], s.w = w[N - 1];
            *reinterpret_cast<Stored4*>(row + at) = s;
        } else {
            Stored2 s;
            s.x = w[0], s.y = w[1];
            *reinterpret_cast<Stored2*>(row + at) = s;
        }
#else
        memcpy(row + at, w, 4 * N);
#endif
        d = N;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 0; e <= N; e++) {
        if (e < d || e >= n) continue;
        const int lo = at + 4 * e;
        if (lo >= 0 && lo + 4 <= nbytes) store_dword(row + lo, w[e]);
        else
            for (int i = 0; i < 4; i++)
                if (lo + i >= 0 && lo + i < nbytes) row[lo + i] = (uint8_t) (w[e] >> (8 * i));
    }
}

// The four streams of a lane, after run(): shifted in with the previous lane's last dwords and stored.  g: the lane's number along the row
// pair; W, cw: the bytes of a Y row and of a chroma row; m*: the streams' addresses modulo 4; ybot: nullptr without a bottom row.
struct Streams {
    uint8_t *ytop, *ybot, *cb, *cr;
    uint32_t m_ytop, m_ybot, m_cb, m_cr;
};

KBE_YUV_HD void store_run(const Streams& s, int g, int W, int cw, const uint32_t (&ytop)[4], const uint32_t (&ybot)[4], const uint32_t (&cb)[2], const uint32_t (&cr)[2],
                          uint32_t prev_ytop, uint32_t prev_ybot, uint32_t prev_cb, uint32_t prev_cr)
{
    // the stream's last lane stores its own last m bytes as well: the dword behind its N
    const int last = kRun * (g + 1) >= W ? 1 : 0;
    uint32_t y[5], c[3];
    shift_in<4>(ytop, prev_ytop, s.m_ytop, y);
    store_piece<4>(s.ytop, W, kRun * g - (int) s.m_ytop, y, 4 + (s.m_ytop ? last : 0));
    if (s.ybot) {
        shift_in<4>(ybot, prev_ybot, s.m_ybot, y);
        store_piece<4>(s.ybot, W, kRun * g - (int) s.m_ybot, y, 4 + (s.m_ybot ? last : 0));
    }
    shift_in<2>(cb, prev_cb, s.m_cb, c);
    store_piece<2>(s.cb, cw, kCells * g - (int) s.m_cb, c, 2 + (s.m_cb ? last : 0));
    shift_in<2>(cr, prev_cr, s.m_cr, c);
    store_piece<2>(s.cr, cw, kCells * g - (int) s.m_cr, c, 2 + (s.m_cr ? last : 0));
}

#if !defined(__HIPCC__)
// One frame on a CPU, serially, the way the kernel takes it: row pair by row pair, lane by lane.  The alignments are GIVEN, so that a test can
// walk through all of them: src_class = the address of the source's first byte, out_class = that of the payload's first byte (any numbers
// congruent to them modulo 16).  The aligned source dwords are kbe_rows.h's aligned_dwords -- 0 where the row has no byte or the dword is
// not loaded --, so nothing outside a row is read; the payload is written through store_piece alone.
inline void convert_frame(const uint8_t* src, long stride, long W, long H, int flags, uint32_t src_class, uint32_t out_class, uint8_t* out)
{
    const Coef k = coef(flags);
    const long cw = (W + 1) / 2, ch = (H + 1) / 2, row_bytes = 3 * W, lanes = (W + kRun - 1) / kRun;
    for (long cy = 0; cy < ch; cy++) {
        const bool two = 2 * cy + 1 < H;
        const long at_ytop = 2 * cy * W, at_cb = W * H + cy * cw, at_cr = at_cb + cw * ch;
        Streams s;
        s.ytop = out + at_ytop, s.ybot = two ? out + at_ytop + W : nullptr, s.cb = out + at_cb, s.cr = out + at_cr;
        s.m_ytop = (uint32_t) ((out_class + at_ytop) & 3), s.m_ybot = (uint32_t) ((out_class + at_ytop + W) & 3);
        s.m_cb = (uint32_t) ((out_class + at_cb) & 3), s.m_cr = (uint32_t) ((out_class + at_cr) & 3);
        uint32_t prev[4] = {0u, 0u, 0u, 0u};
        for (long g = 0; g < lanes; g++) {
            const long j0 = 4 * kRunDwords * g;
            uint32_t rows[2][kRunDwords];
            for (int r = 0; r < 2; r++) {
                const long y = 2 * cy + (two ? r : 0);
                const uint32_t b = (uint32_t) (((long) src_class + y * stride + j0) & 3);
                uint32_t x[kRunDwords + 1];
                kbe_rows::aligned_dwords<kRunDwords>(src + y * stride, j0, b, row_bytes, x);
                realign<kRunDwords>(x, b, rows[r]);
            }
            const long x0 = kRun * g;
            const int lone = (W & 1) && W - 1 >= x0 && W - 1 < x0 + kRun ? (int) ((W - 1 - x0) / 2) : -1;
            uint32_t ytop[4], ybot[4], cb[2], cr[2];
            run(rows[0], rows[1], lone, k, ytop, ybot, cb, cr);
            store_run(s, (int) g, (int) W, (int) cw, ytop, ybot, cb, cr, prev[0], prev[1], prev[2], prev[3]);
            prev[0] = ytop[3], prev[1] = ybot[3], prev[2] = cb[1], prev[3] = cr[1];
        }
    }
}
#endif

}  // namespace kbe_yuv
