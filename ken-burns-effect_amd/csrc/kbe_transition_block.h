// kbe_transition_block.h -- the project's ONE definition of the transitions of kbe_transition_u8 (include/kbe_transition.h).  Two compilations
// read it: hipcc into the kernel of kbe_transition.hip, and g++ into tests/transition_check.cpp, which holds the packed forms below to the plain
// ones on every input they can meet and runs the rows serially.  The device's bytes are what blend_row below gives
// (tests/test_transition_gpu.py, through the NumPy twin).
//
// One output frame is made of two source frames, `from` and `to`, byte by byte.  No floating point.  With
//     blend(a, b, w) = (a (256 - w) + b w + 128) >> 8             (w in 0..256; at most 255 * 256 + 128 = 65408: 16 bits)
// an output byte is blend(from, to, w), the weight w of the byte's pixel (x, y) by the kind and the frame's progress p in 0..256:
//     dissolve                       w = p
//     wipe right, left, down, up     with (t, L) = (x, W), (W - 1 - x, W), (y, H), (H - 1 - y, H) and the softness s in 1..65535:
//                                    num = p (L + s) - 256 t;  w = 0 if num <= 0, else min(256, num / s) in integer division
//     fade                           through a colour: p <= 128: blend(from, colour byte, 2 p); otherwise blend(colour byte, to, 2 p - 256);
//                                    byte k of a pixel meets (colour >> 8 k) & 255
// p = 0 gives `from` and p = 256 gives `to`, byte for byte: blend(a, b, 0) = a and blend(a, b, 256) = b.
//
// The packed forms, which the kernel uses instead of the plain ones (and which are the plain ones: transition_check brute):
//   * a row is taken in PIECES of 16 bytes, four dwords.  Where the four bytes of a dword have one weight (a whole row has, but for the
//     horizontal wipes), the dword is blended as two 16-bit lanes twice, its even bytes and its odd ones: no carry leaves a lane (blend_dword).
//   * the wipes' division is a multiply-high: with M = ceil(2^40 / s) (magic), floor(num M / 2^40) = floor(num / s) for every num < 2^24,
//     since 0 <= M s - 2^40 < s <= 2^16; num >= 256 s (<= 2^24) is 256 without it (weight).
//   * under the horizontal wipes a piece's bytes lie in up to six pixels.  The pixel x0 of the piece's first byte and that byte's channel r
//     come from one multiply-high (pixel_of: j / 3 for every j < 2^31); the pixel of byte i is x0 + (r + i) / 3, which is i / 3 or
//     i / 3 + 1 -- and (r + i) 11 >> 5 for the last byte's, r + i <= 17.  A lane in the soft edge takes six weights, not sixteen.
//   * a piece whose weights are all 0 or all 256 is a copy of one source: plan() says which sources a piece reads, and the kernel loads no other.
//     The weights of a wipe are monotone along its axis: the first and the last byte's decide.  The fade reads one source.
//   * a piece of a source starts anywhere: kbe_rows.h's realign cuts it out of the five aligned dwords that hold it.
#pragma once
#include "kbe_shutter_block.h"

#define KBE_TRANSITION_HD KBE_SHUTTER_HD

namespace kbe_transition {

using kbe_rows::kMaxSide;
using kbe_rows::kPiece;                       // bytes: what one lane of the kernel loads from a source, and stores
using kbe_rows::realign;
using kbe_shutter::kDwords;

constexpr int kMaxSoftness = 65535;
constexpr int kKinds = 6;
enum Kind : uint32_t { kDissolve = 0, kWipeRight = 1, kWipeLeft = 2, kWipeDown = 3, kWipeUp = 4, kFade = 5 };

// -- the plain forms ---------------------------------------------------------------------------
KBE_TRANSITION_HD uint32_t blend(uint32_t a, uint32_t b, uint32_t w)
{
    return (a * (256u - w) + b * w + 128u) >> 8;
}

// a wipe's weight at the place t of the L along its axis, by the plain division
KBE_TRANSITION_HD uint32_t weight_plain(uint32_t p, uint32_t L, uint32_t s, long t)
{
    const long num = (long) p * (long) (L + s) - 256l * t;
    if (num <= 0) return 0u;
    const long q = num / (long) s;
    return q > 256 ? 256u : (uint32_t) q;
}

// -- the packed forms --------------------------------------------------------------------------
// M = ceil(2^40 / s), 1 <= s <= 65535
KBE_TRANSITION_HD uint64_t magic(uint32_t s)
{
    return ((1ull << 40) + (uint64_t) s - 1u) / (uint64_t) s;
}

// weight_plain by the multiply-high; t may lie outside 0..L-1 by a few places (a piece's bytes beyond its row): the same formula goes on
KBE_TRANSITION_HD uint32_t weight(uint32_t p, uint32_t L, uint32_t s, uint64_t M, int32_t t)
{
    const int32_t num = (int32_t) (p * (L + s)) - 256 * t;                  // p (L + s) <= 256 * 131070 < 2^25
    if (num <= 0) return 0u;
    if ((uint32_t) num >= 256u * s) return 256u;
    return (uint32_t) (((uint64_t) (uint32_t) num * M) >> 40);
}

// j / 3 for 0 <= j < 2^31
KBE_TRANSITION_HD uint32_t pixel_of(uint32_t j)
{
    return kbe_shutter::mul_hi(j, 0xAAAAAAABu) >> 1;
}

// four bytes of one weight: blend(a, b, w) of every byte of the dwords a and b
KBE_TRANSITION_HD uint32_t blend_dword(uint32_t a, uint32_t b, uint32_t w)
{
    const uint32_t v = 256u - w;
    const uint32_t even = (a & 0x00FF00FFu) * v + (b & 0x00FF00FFu) * w + 0x00800080u;
    const uint32_t odd = ((a >> 8) & 0x00FF00FFu) * v + ((b >> 8) & 0x00FF00FFu) * w + 0x00800080u;
    return ((even >> 8) & 0x00FF00FFu) | (odd & 0xFF00FF00u);
}

// the dword of colour bytes whose first byte is channel k = 0..2
KBE_TRANSITION_HD uint32_t colour_dword(uint32_t colour, uint32_t k)
{
    const uint64_t c = (uint64_t) (colour & 0xFFFFFFu);
    return (uint32_t) ((c | (c << 24) | (c << 48)) >> (8u * k));
}

// what does not change over a frame
struct Frame {
    uint32_t kind, p, s, colour, W, H;
    uint64_t M;                               // magic(s)
};

// what a lane knows of its piece before it loads anything
struct Plan {
    uint32_t w;                               // the weight of every byte, where `uniform`; under the fade that of the pair the piece blends
    int32_t x0;                               // horizontal wipes: the pixel of the piece's first byte (it may be -1 .. -5 before the row) ...
    uint32_t r;                               // ... and the channel 0..2 of that byte (the fade reads it too)
    bool uniform, from, to;                   // from, to: the sources the piece reads
};

// j0: the piece's first byte as a byte of the row, -15 <= j0 < 3 W; y: its row
KBE_TRANSITION_HD Plan plan(const Frame& f, long j0, uint32_t y)
{
    Plan q;
    const uint32_t jj = (uint32_t) (j0 + 18), third = pixel_of(jj);         // (18: a multiple of 3 that makes it positive)
    q.x0 = (int32_t) third - 6;
    q.r = jj - 3u * third;
    q.uniform = true;
    q.w = f.p;
    if (f.kind == kWipeRight || f.kind == kWipeLeft) {
        const int32_t x1 = q.x0 + (int32_t) (((q.r + 15u) * 11u) >> 5);     // the pixel of the piece's last byte
        const uint32_t w0 = weight(f.p, f.W, f.s, f.M, f.kind == kWipeRight ? q.x0 : (int32_t) f.W - 1 - q.x0);
        const uint32_t w1 = weight(f.p, f.W, f.s, f.M, f.kind == kWipeRight ? x1 : (int32_t) f.W - 1 - x1);
        q.uniform = w0 == w1 && (w0 == 0u || w0 == 256u);                   // (monotone between the two)
        q.w = w0;
    } else if (f.kind == kWipeDown || f.kind == kWipeUp) {
        q.w = weight(f.p, f.H, f.s, f.M, f.kind == kWipeDown ? (int32_t) y : (int32_t) f.H - 1 - (int32_t) y);
    }
    if (f.kind == kFade) {
        q.from = f.p <= 128u;
        q.to = !q.from;
        q.w = q.from ? 2u * f.p : 2u * f.p - 256u;
    } else {
        q.from = !(q.uniform && q.w == 256u);
        q.to = !(q.uniform && q.w == 0u);
    }
    return q;
}

// the four output dwords of a piece from its sources' (a: from, b: to; a source the plan does not read: whatever is there)
KBE_TRANSITION_HD void blend_piece(const Frame& f, const Plan& q, const uint32_t a[4], const uint32_t b[4], uint32_t out[4])
{
    if (f.kind == kFade) {
        for (uint32_t d = 0; d < 4u; d++) {
            const uint32_t k = q.r + d >= 3u ? q.r + d - 3u : q.r + d, c = colour_dword(f.colour, k);    // (4 d = d modulo 3; r + d <= 5)
            out[d] = q.from ? blend_dword(a[d], c, q.w) : blend_dword(c, b[d], q.w);
        }
    } else if (q.uniform) {
        for (int d = 0; d < 4; d++) out[d] = q.w == 0u ? a[d] : q.w == 256u ? b[d] : blend_dword(a[d], b[d], q.w);
    } else {
        // the piece's 16 bytes lie in the pixels x0 .. x0 + 5: six weights, and byte i takes the one of pixel (r + i) / 3 = i / 3 or i / 3 + 1
        // -- a choice between two registers that are known when this is compiled, not a register indexed by a variable
        uint32_t wx[6];
        for (int32_t k = 0; k < 6; k++) wx[k] = weight(f.p, f.W, f.s, f.M, f.kind == kWipeRight ? q.x0 + k : (int32_t) f.W - 1 - q.x0 - k);
        for (uint32_t d = 0; d < 4u; d++) {
            uint32_t word = 0u;
            for (uint32_t e = 0; e < 4u; e++) {
                const uint32_t i = 4u * d + e, next = i / 3u + 1u > 5u ? 5u : i / 3u + 1u;                     // (only i = 15, whose i % 3 is 0: never taken)
                const uint32_t w = (i % 3u) + q.r >= 3u ? wx[next] : wx[i / 3u];
                word |= blend((a[d] >> (8u * e)) & 255u, (b[d] >> (8u * e)) & 255u, w) << (8u * e);
            }
            out[d] = word;
        }
    }
}

#if !defined(__HIPCC__)
// One output row on a CPU, serially, the way the kernel takes it: pieces of 16 bytes at the OUTPUT row's alignment (`lead` = its address
// modulo 16, given by the caller so that a test can walk through all sixteen), each source realigned by its own address modulo 4
// (from_class, to_class: the address of the source row's first byte, any number congruent to it modulo 4).  The walk over the pieces, the
// aligned dwords of a row and the store of a piece are kbe_rows.h's: nothing outside a row is read or written; a source that the plan does
// not read is not looked at: its dwords are 0xDD.
inline void source_piece(const uint8_t* row, uint32_t row_class, bool read, long j0, long row_bytes, uint32_t (&w)[kDwords])
{
    const uint32_t b = (uint32_t) (((long) row_class + j0) & 3);
    uint32_t x[kDwords + 1];
    if (read) kbe_rows::aligned_dwords<kDwords>(row, j0, b, row_bytes, x);
    else memset(x, 0xDD, sizeof(x));
    realign(x, b, w);
}

inline void blend_row(const Frame& f, const uint8_t* from, const uint8_t* to, uint32_t from_class, uint32_t to_class, uint32_t y, uint32_t lead, uint8_t* out)
{
    const long row_bytes = 3l * (long) f.W;
    kbe_rows::for_each_piece(row_bytes, lead, [&](uint32_t at) {
        const long j0 = (long) at - (long) lead;
        const Plan q = plan(f, j0, y);
        uint32_t a[4], b[4], word[4];
        source_piece(from, from_class, q.from, j0, row_bytes, a);
        source_piece(to, to_class, q.to, j0, row_bytes, b);
        blend_piece(f, q, a, b, word);
        kbe_rows::store_piece(out, lead, lead + (uint32_t) row_bytes, at, word);
    });
}
#endif

}  // namespace kbe_transition
