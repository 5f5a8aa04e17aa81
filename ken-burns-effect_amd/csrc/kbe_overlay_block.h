// kbe_overlay_block.h -- the project's ONE definition of the compositing of kbe_overlay_u8 (include/kbe_overlay.h).  Two compilations read it:
// hipcc into the kernel of kbe_overlay.hip, and g++ into tests/overlay_check.cpp, which holds the packed forms below to the plain ones on
// every input they can meet and runs the rows serially.  The device's bytes are what over_row below gives (tests/test_overlay_gpu.py,
// through the NumPy twin).
//
// An RGBA picture over 3-byte pixels, in place.  No floating point.  For a frame byte c, the overlay byte o of the same channel, the
// overlay pixel's alpha a and the frame's opacity in 0..256:
//     e   = (a * opacity + 128) >> 8                  (0..255: at most 255 * 256 + 128 = 65408)
//     out = (c * (255 - e) + o * e + 127) / 255       (integer division; the numerator is at most 255 * 255 + 127 = 65152: 16 bits)
// e = 0 gives c, e = 255 gives o, c == o gives c.
//
// The packed forms, which the kernel uses instead of the plain ones (and which are the plain ones: overlay_check brute):
//   * the division: with m = n + 1, n / 255 = (m + (m >> 8)) >> 8 for every n <= 65152 (it is floor(257 m / 65536), and 65536 / 257 lies
//     0.004 above 255).  m = c (255 - e) + o e + 128 and m + (m >> 8) <= 65153 + 254 both fit 16 bits;
//   * so two bytes are composited in the two 16-bit lanes of a dword, each with an e of its own (Pair: a vector of two uint16_t, which
//     both compilers know; the chip multiplies and adds its two lanes in one instruction each), and a dword of four frame bytes takes two
//     such steps, its even bytes and its odd ones (over_dword);
//   * a row of the clipped rectangle is taken in PIECES of 16 frame bytes, four dwords, at the alignment of the frame's bytes.  A piece's
//     bytes lie in six pixels, starting at the channel r = 0..2 of the first (first_pixel: one multiply-high).  The six overlay pixels, 24
//     bytes that start anywhere, are cut out of the seven aligned dwords that hold them (realign); their colour bytes are packed into a
//     stream of 18 bytes, pixel k at byte 3 k (colour_stream), their six e, each three times, into another, and both streams are moved by r
//     bytes: then byte i of the piece meets byte i of both (over_piece).  Nothing is indexed by a variable.
#pragma once
#include "kbe_shutter_block.h"

#define KBE_OVERLAY_HD KBE_SHUTTER_HD

namespace kbe_overlay {

using kbe_rows::align_bytes;
using kbe_rows::frame_dword_holds_a_byte;
using kbe_rows::kMaxSide;
using kbe_rows::kPiece;                       // bytes of a frame: what one lane of the kernel loads, composites and stores
using kbe_rows::realign;                      // (the six overlay pixels, 24 bytes that start b bytes into the 28 bytes x[0..6])
using kbe_shutter::mul_hi;

constexpr int kMaxOpacity = 256;
constexpr int kPixels = 6;                    // the pixels that hold a piece's bytes

// -- the plain forms ---------------------------------------------------------------------------
KBE_OVERLAY_HD uint32_t effective(uint32_t a, uint32_t opacity)
{
    return (a * opacity + 128u) >> 8;
}

KBE_OVERLAY_HD uint32_t over(uint32_t c, uint32_t o, uint32_t e)
{
    return (c * (255u - e) + o * e + 127u) / 255u;
}

// -- the packed forms --------------------------------------------------------------------------
typedef uint16_t Pair __attribute__((vector_size(4)));      // two 16-bit lanes of one dword

KBE_OVERLAY_HD Pair pair_of(uint32_t v)
{
    Pair p;
    __builtin_memcpy(&p, &v, 4);
    return p;
}

KBE_OVERLAY_HD uint32_t word_of(Pair p)
{
    uint32_t v;
    __builtin_memcpy(&v, &p, 4);
    return v;
}

// n / 255 from m = n + 1, for n <= 65152
KBE_OVERLAY_HD uint32_t div255(uint32_t m)
{
    return (m + (m >> 8)) >> 8;
}

// over() in both lanes, every lane with its own c, o and e in 0..255
KBE_OVERLAY_HD Pair over_pair(Pair c, Pair o, Pair e)
{
    const Pair full = {255, 255}, half = {128, 128};
    const Pair m = c * (full - e) + o * e + half;
    return (m + (m >> 8)) >> 8;
}

// over() of the four bytes of c with the four bytes of o, byte i at the e in byte i of `e`
KBE_OVERLAY_HD uint32_t over_dword(uint32_t c, uint32_t o, uint32_t e)
{
    const uint32_t even = word_of(over_pair(pair_of(c & 0x00FF00FFu), pair_of(o & 0x00FF00FFu), pair_of(e & 0x00FF00FFu)));
    const uint32_t odd = word_of(over_pair(pair_of((c >> 8) & 0x00FF00FFu), pair_of((o >> 8) & 0x00FF00FFu), pair_of((e >> 8) & 0x00FF00FFu)));
    return even | (odd << 8);
}

// the pixel x0 of the byte j0 of a row of 3-byte pixels and that byte's channel r, -15 <= j0 < 3 * 65535 (x0 = -1 .. -5 before the row)
KBE_OVERLAY_HD void first_pixel(long j0, int32_t* x0, uint32_t* r)
{
    const uint32_t jj = (uint32_t) (j0 + 18), third = mul_hi(jj, 0xAAAAAAABu) >> 1;      // (18: a multiple of 3 that makes it positive)
    *x0 = (int32_t) third - 6;
    *r = jj - 3u * third;
}

// The six overlay pixels x0 .. x0 + 5 of a row of the rectangle are 24 bytes that begin b bytes into the first of seven ALIGNED dwords;
// dword m covers the bytes 4 m - b .. 4 m - b + 3 of them.  The rectangle's row has `pixels` pixels, and a piece reads those of its six
// that lie in it: a dword that holds no byte of such a pixel is not loaded -- its address may not exist.  Nothing is taken from dword 6
// where b = 0.
KBE_OVERLAY_HD bool overlay_dword_holds_a_byte(int32_t x0, uint32_t b, int m, int32_t pixels)
{
    const int32_t first = x0 < 0 ? -x0 : 0, last = pixels - 1 - x0 < kPixels - 1 ? pixels - 1 - x0 : kPixels - 1;
    const int32_t at = 4 * m - (int32_t) b;
    return at < 4 * last + 4 && at + 4 > 4 * first;
}

// ... and whether all seven do, whatever b is
KBE_OVERLAY_HD bool all_overlay_dwords_hold_a_byte(int32_t x0, int32_t pixels)
{
    return x0 >= 0 && x0 + kPixels < pixels;
}

// bytes 0..2 of six dwords as a stream of 18 bytes, those of dword k at byte 3 k (the last two bytes of s[4] are 0)
KBE_OVERLAY_HD void colour_stream(const uint32_t p[6], uint32_t s[5])
{
    s[0] = (p[0] & 0xFFFFFFu) | (p[1] << 24);
    s[1] = ((p[1] >> 8) & 0xFFFFu) | (p[2] << 16);
    s[2] = ((p[2] >> 16) & 0xFFu) | (p[3] << 8);
    s[3] = (p[4] & 0xFFFFFFu) | (p[5] << 24);
    s[4] = (p[5] >> 8) & 0xFFFFu;
}

// The four output dwords of a piece: its frame bytes c, its six overlay pixels (a pixel outside the rectangle: whatever is there), the
// channel r of its first byte.  -> the four dwords of e OR-ed: 0 says that the piece is what it was
KBE_OVERLAY_HD uint32_t over_piece(const uint32_t pixel[6], uint32_t opacity, uint32_t r, const uint32_t c[4], uint32_t out[4])
{
    uint32_t thrice[6], colours[5], weights[5];
    for (int k = 0; k < kPixels; k++) thrice[k] = effective(pixel[k] >> 24, opacity) * 0x010101u;
    colour_stream(pixel, colours);
    colour_stream(thrice, weights);
    uint32_t any = 0u;
    for (int d = 0; d < 4; d++) {
        const uint32_t o = align_bytes(colours[d + 1], colours[d], r), e = align_bytes(weights[d + 1], weights[d], r);
        out[d] = over_dword(c[d], o, e);
        any |= e;
    }
    return any;
}

#if !defined(__HIPCC__)
// One row of the clipped rectangle on a CPU, serially and in place, the way the kernel takes it: pieces of 16 bytes at the alignment of the
// frame's bytes (`lead` = the address of the row's first byte modulo 16, given by the caller so that a test can walk through all sixteen),
// the overlay's pixels realigned by their address modulo 4 (overlay_class: the address of the row's first overlay pixel, any number
// congruent to it modulo 4).  The aligned dwords are put together byte by byte from the rows alone -- 0 where a row has no byte or the
// dword is not loaded --, so nothing outside the rows is read; a piece whose e are all 0 is not written.  The walk over the pieces, a
// piece's bounds and its store are kbe_rows.h's.
inline void over_row(uint8_t* frame, const uint8_t* overlay, uint32_t overlay_class, int32_t pixels, uint32_t opacity, uint32_t lead)
{
    const long row_bytes = 3l * pixels;
    kbe_rows::for_each_piece(row_bytes, lead, [&](uint32_t at) {
        const long j0 = (long) at - (long) lead;
        const kbe_rows::Piece q = kbe_rows::piece_of(frame, lead, lead + (uint32_t) row_bytes, at);
        int32_t x0;
        uint32_t r;
        first_pixel(j0, &x0, &r);
        const uint32_t b = (uint32_t) (((long) overlay_class + 4l * x0) & 3);
        const bool all = all_overlay_dwords_hold_a_byte(x0, pixels);
        uint8_t bytes[28], mine[16];
        for (long i = 0; i < 28; i++) {
            const long j = 4l * x0 - (long) b + i;                               // as a byte of the overlay's row
            const bool loaded = all || overlay_dword_holds_a_byte(x0, b, (int) (i / 4), pixels);
            bytes[i] = loaded && j >= 0 && j < 4l * pixels ? overlay[j] : (uint8_t) 0;
        }
        for (long i = 0; i < 16; i++) {
            const bool loaded = q.whole() || frame_dword_holds_a_byte((uint32_t) (i / 4), q.lo, q.hi);
            mine[i] = loaded && j0 + i >= 0 && j0 + i < row_bytes ? frame[j0 + i] : (uint8_t) 0;
        }
        uint32_t x[7], pixel[6], c[4], word[4];
        memcpy(x, bytes, 28);
        memcpy(c, mine, 16);
        realign(x, b, pixel);
        if (over_piece(pixel, opacity, r, c, word) == 0u) return;
        kbe_rows::store_piece(frame, lead, lead + (uint32_t) row_bytes, at, word);
    });
}
#endif

}  // namespace kbe_overlay
