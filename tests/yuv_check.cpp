// yuv_check.cpp -- csrc/kbe_yuv_block.h compiled by g++ and executed serially: the packed forms the kernel of kbe_yuv420_u8 computes with, held
// to the plain definition (tests/test_yuv_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   yuv_check brute
//       for all 2^24 (R, G, B), in both channel orders: luma_word's byte 1 is luma_of, and chroma_of on the pixel four times is cb_of / cr_of
//       at n = 1, whatever byte 3 of the pixel's dword holds; cells of n = 2 and n = 4 pixels -- every combination of the eight corners of
//       the colour cube, and random ones -- against cb_of / cr_of on their sums; bytes1, realign and shift_in against the bytes themselves;
//       whole frames through convert_frame, W and H in 1..9 and widths around one and two lanes' runs, at every pair of classes of the source
//       and the payload modulo 16, against the plain form pixel by pixel and cell by cell, with the bytes around the payload looked at.
//   yuv_check convert W H stride flags n in.raw out.raw
//       in.raw: n frames [H][stride] bytes back to back; out.raw: n payloads.  Frame i is taken at the class of its offset in the file and
//       its payload at the class (5 i + 3) % 16: every frame another.
//   yuv_check bytes W H
//       kbe_yuv_block.h's payload_bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_yuv_block.h"

using namespace kbe_yuv;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 8;
}

// the plain form of a whole frame: pixel by pixel, cell by cell
static void plain_frame(const uint8_t* src, long stride, long W, long H, int flags, uint8_t* out)
{
    const long cw = (W + 1) / 2, ch = (H + 1) / 2;
    const int r = flags & kFlagBGR ? 2 : 0, b = 2 - r;
    for (long y = 0; y < H; y++)
        for (long x = 0; x < W; x++) {
            const uint8_t* p = src + y * stride + 3 * x;
            out[y * W + x] = (uint8_t) luma_of(p[r], p[1], p[b]);
        }
    for (long cy = 0; cy < ch; cy++)
        for (long cx = 0; cx < cw; cx++) {
            int Rs = 0, Gs = 0, Bs = 0, n = 0;
            for (long y = 2 * cy; y < 2 * cy + 2 && y < H; y++)
                for (long x = 2 * cx; x < 2 * cx + 2 && x < W; x++, n++) {
                    const uint8_t* p = src + y * stride + 3 * x;
                    Rs += p[r], Gs += p[1], Bs += p[b];
                }
            const int log2n = n == 4 ? 2 : n == 2 ? 1 : 0;
            out[W * H + cy * cw + cx] = (uint8_t) cb_of(Rs, Gs, Bs, log2n);
            out[W * H + cw * ch + cy * cw + cx] = (uint8_t) cr_of(Rs, Gs, Bs, log2n);
        }
}

static uint32_t dword_of(uint32_t R, uint32_t G, uint32_t B, int flags, uint32_t junk)
{
    return flags & kFlagBGR ? B | G << 8 | R << 16 | junk << 24 : R | G << 8 | B << 16 | junk << 24;
}

static int brute()
{
    long luma_bad = 0, one_bad = 0, two_bad = 0, four_bad = 0, range_bad = 0, pack_bad = 0, frame_bad = 0, pixels = 0, twos = 0, fours = 0, frames = 0;
    for (int flags = 0; flags < 2; flags++) {
        const Coef k = coef(flags);
        for (uint32_t v = 0; v < (1u << 24); v++, pixels++) {
            const uint32_t R = v & 255u, G = (v >> 8) & 255u, B = v >> 16, p = dword_of(R, G, B, flags, (v * 2654435761u) >> 24);
            const uint32_t Y = luma_of(R, G, B), U = cb_of((int) R, (int) G, (int) B, 0), V = cr_of((int) R, (int) G, (int) B, 0);
            if (((luma_word(p, k.wy) >> 8) & 255u) != Y || luma_word(p, k.wy) >> 16) luma_bad++;
            if (chroma_of(p, p, p, p, k.wcb, k.xcb) != U || chroma_of(p, p, p, p, k.wcr, k.xcr) != V) one_bad++;
            if (Y < 16u || Y > 235u || U < 16u || U > 240u || V < 16u || V > 240u) range_bad++;
        }
        // n = 2 and n = 4: the corners of the cube in every combination, then random pixels
        uint32_t state = 11u + (uint32_t) flags;
        for (long i = 0; i < 64 + 4096 + 2000000; i++) {
            uint32_t c[4][3];
            const int n = i < 64 ? 2 : i < 64 + 4096 ? 4 : 2 + 2 * (int) (i & 1);
            for (int q = 0; q < 4; q++)
                for (int ch = 0; ch < 3; ch++) {
                    if (i < 64) c[q][ch] = ((i >> (3 * q + ch)) & 1) ? 255u : 0u;
                    else if (i < 64 + 4096) c[q][ch] = (((i - 64) >> (3 * q + ch)) & 1) ? 255u : 0u;
                    else c[q][ch] = lcg(&state) & 255u;
                }
            int Rs = 0, Gs = 0, Bs = 0;
            uint32_t p[4];
            for (int q = 0; q < n; q++) Rs += (int) c[q][0], Gs += (int) c[q][1], Bs += (int) c[q][2], p[q] = dword_of(c[q][0], c[q][1], c[q][2], flags, lcg(&state) & 255u);
            const uint32_t U = cb_of(Rs, Gs, Bs, n == 4 ? 2 : 1), V = cr_of(Rs, Gs, Bs, n == 4 ? 2 : 1);
            const bool ok = n == 4 ? chroma_of(p[0], p[1], p[2], p[3], k.wcb, k.xcb) == U && chroma_of(p[0], p[1], p[2], p[3], k.wcr, k.xcr) == V
                                   : chroma_of(p[0], p[0], p[1], p[1], k.wcb, k.xcb) == U && chroma_of(p[0], p[1], p[0], p[1], k.wcr, k.xcr) == V;
            if (n == 4) fours++, four_bad += ok ? 0 : 1;
            else twos++, two_bad += ok ? 0 : 1;
            if (U < 16u || U > 240u || V < 16u || V > 240u) range_bad++;
        }
    }
    {   // bytes1, realign, shift_in: against the bytes themselves
        if (bytes1(0x00AA11u, 0xFFBB22u, 0x12CC33u, 0x00DD44u) != 0xDDCCBBAAu) pack_bad++;
        uint8_t bytes[4 * (kRunDwords + 1)];
        for (size_t i = 0; i < sizeof(bytes); i++) bytes[i] = (uint8_t) (17 * i + 3);
        for (uint32_t b = 0; b < 4u; b++) {
            uint32_t x[kRunDwords + 1], w[kRunDwords];
            memcpy(x, bytes, sizeof(x));
            realign<kRunDwords>(x, b, w);
            if (memcmp(w, bytes + b, sizeof(w)) != 0) pack_bad++;
            for (int i = 0; i < kRun; i++) {
                uint32_t want = 0;
                memcpy(&want, bytes + b + 3 * i, i + 1 < kRun ? 4 : 3);
                if (pixel(w, i) != want) pack_bad++;
            }
        }
        for (uint32_t m = 0; m < 4u; m++) {
            // the stream: prev's four bytes, then own's 16; shifted in, the lane's dwords begin m bytes before its own
            uint32_t prev, own[4], out[5];
            memcpy(&prev, bytes, 4);
            memcpy(own, bytes + 4, 16);
            shift_in<4>(own, prev, m, out);
            if (memcmp(out, bytes + 4 - m, 16 + m) != 0) pack_bad++;
        }
    }
    // whole frames
    uint32_t state = 5u;
    const long widths[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47};
    for (long W : widths)
        for (long H = 1; H <= 9; H++) {
            if (W > 9 && H > 3) continue;
            const long stride = 3 * W + 1 + (W + H) % 3, bytes = (long) payload_bytes(W, H);
            std::vector<uint8_t> src((size_t) (H * stride)), want((size_t) bytes), got((size_t) bytes + 8);
            for (uint32_t src_class = 0; src_class < 16u; src_class++)
                for (uint32_t out_class = 0; out_class < 16u; out_class++, frames++) {
                    const int flags = (int) ((src_class + out_class) & 1u);
                    for (auto& v : src) v = (uint8_t) lcg(&state);
                    plain_frame(src.data(), stride, W, H, flags, want.data());
                    memset(got.data(), 0xEE, got.size());
                    convert_frame(src.data(), stride, W, H, flags, src_class, out_class, got.data() + 4);
                    bool ok = memcmp(got.data() + 4, want.data(), (size_t) bytes) == 0;
                    for (int i = 0; i < 4; i++) ok = ok && got[(size_t) i] == 0xEE && got[(size_t) (bytes + 4 + i)] == 0xEE;
                    if (!ok) frame_bad++;
                }
        }
    printf("brute: pixels %ld, luma mismatches %ld, chroma mismatches %ld, pairs %ld, pair mismatches %ld, fours %ld, four mismatches %ld, out of range %ld, "
           "packing mismatches %ld, frames %ld, frame mismatches %ld\n", pixels, luma_bad, one_bad, twos, two_bad, fours, four_bad, range_bad, pack_bad, frames, frame_bad);
    return luma_bad || one_bad || two_bad || four_bad || range_bad || pack_bad || frame_bad ? 1 : 0;
}

static int convert(int argc, char** argv)
{
    if (argc != 9) return 2;
    const long W = atol(argv[2]), H = atol(argv[3]), stride = atol(argv[4]), flags = atol(argv[5]), n = atol(argv[6]);
    if (W < 1 || W > kMaxSide || H < 1 || H > kMaxSide || stride < 3 * W || (flags & ~(long) kFlagBGR) || n < 1) return 2;
    const size_t bytes = payload_bytes(W, H);
    std::vector<uint8_t> in((size_t) n * H * stride), out((size_t) n * bytes);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
    fclose(f);
    for (long i = 0; i < n; i++) {
        const size_t at = (size_t) i * H * stride;
        convert_frame(in.data() + at, stride, W, H, (int) flags, (uint32_t) (at & 15u), (uint32_t) ((5 * i + 3) % 16), out.data() + (size_t) i * bytes);
    }
    f = fopen(argv[8], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "brute")) return brute();
    if (argc >= 2 && !strcmp(argv[1], "convert")) return convert(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "bytes")) return printf("%zu\n", payload_bytes(atol(argv[2]), atol(argv[3]))) < 0;
    fprintf(stderr, "usage: yuv_check brute | convert W H stride flags n in.raw out.raw | bytes W H\n");
    return 2;
}
