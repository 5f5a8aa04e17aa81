// overlay_check.cpp -- csrc/kbe_overlay_block.h compiled by g++ and executed serially: the packed forms the kernel of kbe_overlay_u8 computes
// with, held to the plain definition (tests/test_overlay_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   overlay_check brute
//       all 256 x 256 x 256 (c, o, e): the plain form in range, over(c, o, 0) = c, over(c, o, 255) = o, over(c, c, e) = c, the division
//       without a divide, and over_dword in every lane of a dword against it; all 256 x 257 (a, opacity): e in 0..255, 0 at opacity 0, a at
//       opacity 256, and a piece whose pixels carry that alpha through over_piece against the plain forms; first_pixel for every first byte
//       -15 .. 3 * 65535 - 1; colour_stream against the bytes; whole rows, lane by lane (over_row), at all 64 pairs of classes of the frame
//       and the overlay and widths from 1 pixel on, against the plain form byte by byte.
//   overlay_check over W H stride n w h overlay_stride x0,x1,... y0,y1,... o0,o1,... in.raw out.raw
//       in.raw: the n frames, [H][stride] bytes each, back to back, then the overlay, [h][overlay_stride] bytes; out.raw: the n frames as
//       they are afterwards, padding included.  A row of the rectangle is taken at the class of its first byte's offset in the file, the
//       overlay's at the class of its offset in the overlay.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_overlay_block.h"

using namespace kbe_overlay;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 24;
}

// the definition, written out
static uint32_t plain_e(uint32_t a, uint32_t opacity)
{
    return (a * opacity + 128u) / 256u;
}

static uint8_t plain_byte(uint32_t c, uint32_t o, uint32_t a, uint32_t opacity)
{
    const uint32_t e = plain_e(a, opacity);
    return (uint8_t) ((c * (255u - e) + o * e + 127u) / 255u);
}

static int brute()
{
    long overs = 0, plain_bad = 0, packed_bad = 0, alphas = 0, alpha_bad = 0, thirds = 0, third_bad = 0, stream_bad = 0, rows = 0, row_bad = 0;
    for (uint32_t c = 0; c < 256u; c++)
        for (uint32_t o = 0; o < 256u; o++)
            for (uint32_t e = 0; e < 256u; e++, overs++) {
                const uint32_t n = c * (255u - e) + o * e + 127u, v = over(c, o, e);
                if (v != n / 255u || v > 255u || n > 65152u || (e == 0u && v != c) || (e == 255u && v != o) || (c == o && v != c) || div255(n + 1u) != v) plain_bad++;
                // the nearest value: |255 v - (c (255 - e) + o e)| <= 127
                const long exact = (long) c * (255 - (long) e) + (long) o * e, off = 255l * v - exact;
                if (off > 127 || off < -127) plain_bad++;
                // every lane of a dword with values of its own
                const uint32_t C = c | ((255u - c) << 8) | (o << 16) | (e << 24), O = o | ((255u - o) << 8) | (e << 16) | (c << 24), E = e | ((255u - e) << 8) | (c << 16) | (o << 24);
                const uint32_t want = v | (over(255u - c, 255u - o, 255u - e) << 8) | (over(o, e, c) << 16) | (over(e, c, o) << 24);
                if (over_dword(C, O, E) != want) packed_bad++;
            }
    for (uint32_t a = 0; a < 256u; a++)
        for (uint32_t opacity = 0; opacity <= 256u; opacity++, alphas++) {
            const uint32_t e = effective(a, opacity);
            if (e != plain_e(a, opacity) || e > 255u || (opacity == 0u && e != 0u) || (opacity == 256u && e != a) || (a == 0u && e != 0u)) alpha_bad++;
            // a piece of six pixels of this alpha and of 255 - a in turn, at every channel of its first byte
            uint32_t pixel[6], c[4], out[4];
            uint8_t frame[16], got[16];
            for (uint32_t k = 0; k < 6u; k++) pixel[k] = ((k & 1u ? 255u - a : a) << 24) | ((17u * k + a) & 255u) | (((opacity + 31u * k) & 255u) << 8) | (((a ^ (opacity + k)) & 255u) << 16);
            for (uint32_t i = 0; i < 16u; i++) frame[i] = (uint8_t) (a + 13u * i + opacity);
            memcpy(c, frame, 16);
            for (uint32_t r = 0; r < 3u; r++) {
                const uint32_t any = over_piece(pixel, opacity, r, c, out);
                memcpy(got, out, 16);
                bool zero = true;
                for (uint32_t i = 0; i < 16u; i++) {
                    const uint32_t k = (r + i) / 3u, ch = (r + i) % 3u;
                    if (got[i] != plain_byte(frame[i], (pixel[k] >> (8u * ch)) & 255u, pixel[k] >> 24, opacity)) alpha_bad++;
                    zero = zero && plain_e(pixel[k] >> 24, opacity) == 0u;
                }
                if (zero != (any == 0u)) alpha_bad++;
            }
        }
    for (long j0 = -15; j0 < 3l * 65535l; j0++, thirds++) {
        int32_t x0;
        uint32_t r;
        first_pixel(j0, &x0, &r);
        const long x = j0 >= 0 ? j0 / 3 : -((-j0 + 2) / 3), rem = j0 - 3 * x;                  // the floor and its remainder
        if (x0 != (int32_t) x || r != (uint32_t) rem) third_bad++;
    }
    {
        uint8_t bytes[24], got[20];
        uint32_t p[6], s[5];
        for (int i = 0; i < 24; i++) bytes[i] = (uint8_t) (i + 1);
        memcpy(p, bytes, 24);
        colour_stream(p, s);
        memcpy(got, s, 20);
        for (int i = 0; i < 18; i++)
            if (got[i] != bytes[4 * (i / 3) + i % 3]) stream_bad++;
        if (got[18] || got[19]) stream_bad++;
    }
    // rows: noise, every class of the frame's row and of the overlay's; the opacity walks through its range
    uint32_t state = 7u;
    const int32_t widths[] = {1, 2, 3, 5, 6, 7, 11, 12, 23, 40};
    const uint32_t opacities[] = {0, 1, 37, 128, 129, 200, 255, 256};
    for (int32_t pixels : widths)
        for (uint32_t lead = 0; lead < 16u; lead++)
            for (uint32_t cls = 0; cls < 4u; cls++, rows++) {
                const uint32_t opacity = opacities[(lead + cls + (uint32_t) pixels) % 8u];
                std::vector<uint8_t> frame(3 * pixels + 2), before, overlay(4 * pixels);
                for (auto& v : frame) v = (uint8_t) lcg(&state);
                for (auto& v : overlay) v = (uint8_t) lcg(&state);
                for (int32_t k = 0; k < pixels; k += 3) overlay[4 * k + 3] = k % 2 ? 0 : 255;      // (alpha 0 and 255 among the noise)
                before = frame;
                over_row(frame.data() + 1, overlay.data(), cls, pixels, opacity, lead);
                bool bad = frame[0] != before[0] || frame[3 * pixels + 1] != before[3 * pixels + 1];
                for (int32_t j = 0; j < 3 * pixels; j++)
                    if (frame[1 + j] != plain_byte(before[1 + j], overlay[4 * (j / 3) + j % 3], overlay[4 * (j / 3) + 3], opacity)) bad = true;
                if (bad) row_bad++;
            }
    printf("brute: overs %ld, plain mismatches %ld, packed mismatches %ld, alphas %ld, alpha mismatches %ld, thirds %ld, third mismatches %ld, "
           "stream mismatches %ld, rows %ld, row mismatches %ld\n", overs, plain_bad, packed_bad, alphas, alpha_bad, thirds, third_bad, stream_bad, rows, row_bad);
    return plain_bad || packed_bad || alpha_bad || third_bad || stream_bad || row_bad ? 1 : 0;
}

static bool numbers(char* at, long n, std::vector<long>* out)
{
    while (*at) {
        out->push_back(strtol(at, &at, 10));
        if (*at == ',') at++;
    }
    return (long) out->size() == n;
}

static int over_frames(int argc, char** argv)
{
    if (argc != 14) return 2;
    const long W = atol(argv[2]), H = atol(argv[3]), stride = atol(argv[4]), n = atol(argv[5]), w = atol(argv[6]), h = atol(argv[7]), ostride = atol(argv[8]);
    if (W < 1 || W > kMaxSide || H < 1 || H > kMaxSide || stride < 3 * W || n < 1 || w < 1 || w > kMaxSide || h < 1 || h > kMaxSide || ostride < 4 * w) return 2;
    std::vector<long> xs, ys, os;
    if (!numbers(argv[9], n, &xs) || !numbers(argv[10], n, &ys) || !numbers(argv[11], n, &os)) return 2;
    std::vector<uint8_t> in((size_t) (n * H * stride + h * ostride));
    FILE* file = fopen(argv[12], "rb");
    if (!file || fread(in.data(), 1, in.size(), file) != in.size()) return 3;
    fclose(file);
    const uint8_t* const overlay = in.data() + n * H * stride;
    for (long i = 0; i < n; i++) {
        if (os[i] < 0 || os[i] > kMaxOpacity || xs[i] < -kMaxSide || xs[i] > kMaxSide || ys[i] < -kMaxSide || ys[i] > kMaxSide) return 2;
        const long x0 = xs[i] > 0 ? xs[i] : 0, x1 = xs[i] + w < W ? xs[i] + w : W, y0 = ys[i] > 0 ? ys[i] : 0, y1 = ys[i] + h < H ? ys[i] + h : H;
        if (os[i] == 0 || x1 <= x0 || y1 <= y0) continue;
        for (long y = y0; y < y1; y++) {
            const size_t frame_at = (size_t) ((i * H + y) * stride + 3 * x0), overlay_at = (size_t) ((y - ys[i]) * ostride + 4 * (x0 - xs[i]));
            over_row(in.data() + frame_at, overlay + overlay_at, (uint32_t) (overlay_at & 3u), (int32_t) (x1 - x0), (uint32_t) os[i], (uint32_t) (frame_at & 15u));
        }
    }
    file = fopen(argv[13], "wb");
    if (!file || fwrite(in.data(), 1, (size_t) (n * H * stride), file) != (size_t) (n * H * stride)) return 3;
    fclose(file);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "brute")) return brute();
    if (argc >= 2 && !strcmp(argv[1], "over")) return over_frames(argc, argv);
    fprintf(stderr, "usage: overlay_check brute | over W H stride n w h overlay_stride x0,x1,... y0,y1,... o0,o1,... in.raw out.raw\n");
    return 2;
}
