// transition_check.cpp -- csrc/kbe_transition_block.h compiled by g++ and executed serially: the packed forms the kernel of kbe_transition_u8
// computes with, held to the plain definition (tests/test_transition_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   transition_check brute
//       all 256 x 256 x 257 blends: the plain form in range, blend(a, b, 0) = a, blend(a, b, 256) = b, and blend_dword in every lane of a
//       dword against it; the wipes' weight by the multiply-high against the plain division for every p in 0..256, L in {1, 2, 5, 50, 341,
//       400, 1366, 65535}, s in {1, 2, 3, 8, 40, 255, 256, 1000, 65535} and every t in -6 .. L + 5; pixel_of(j) = j / 3 for every
//       j < 3 * 65535 + 64, (r + i) 11 >> 5 = (r + i) / 3 up to 17, and plan()'s pixel and channel for every first byte -15 .. 3 * 65535 - 1;
//       colour_dword against the bytes; whole frames of every kind, lane by lane (blend_row), at all 256 pairs of classes of the output and
//       the sources, against the plain form byte by byte.
//   transition_check blend W H stride kind softness colour n p0,p1,... in.raw out.raw
//       in.raw: the n `from` frames and then the n `to` frames, [H][stride] bytes each, back to back; out.raw: n frames [H][3 W].  The
//       output rows are taken at the class (y + i) % 16, the rows of a source at the class of their offset in the file: every row another.
//   transition_check weights W H kind softness p out.raw
//       out.raw: the weight of every pixel as uint16 [H][W], by plan() and weight() the way a lane asks (not for the fade).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_transition_block.h"

using namespace kbe_transition;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 24;
}

// the definition, written out: the byte k of the pixel (x, y)
static uint32_t plain_weight(const Frame& f, long x, long y)
{
    long t, L;
    switch (f.kind) {
    case kWipeRight: t = x, L = f.W; break;
    case kWipeLeft: t = (long) f.W - 1 - x, L = f.W; break;
    case kWipeDown: t = y, L = f.H; break;
    case kWipeUp: t = (long) f.H - 1 - y, L = f.H; break;
    default: return f.p;
    }
    const long num = (long) f.p * (L + (long) f.s) - 256 * t;
    if (num <= 0) return 0u;
    return num / (long) f.s > 256 ? 256u : (uint32_t) (num / (long) f.s);
}

static uint8_t plain_byte(const Frame& f, uint32_t a, uint32_t b, long x, long y, int k)
{
    if (f.kind == kFade) {
        const uint32_t c = (f.colour >> (8 * k)) & 255u;
        return (uint8_t) (f.p <= 128u ? (a * (256u - 2u * f.p) + c * (2u * f.p) + 128u) >> 8
                                      : (c * (256u - (2u * f.p - 256u)) + b * (2u * f.p - 256u) + 128u) >> 8);
    }
    const uint32_t w = plain_weight(f, x, y);
    return (uint8_t) ((a * (256u - w) + b * w + 128u) >> 8);
}

static int brute()
{
    long blends = 0, plain_bad = 0, packed_bad = 0, weights = 0, weight_bad = 0, thirds = 0, third_bad = 0, colour_bad = 0, frames = 0, frame_bad = 0;
    for (uint32_t a = 0; a < 256u; a++)
        for (uint32_t b = 0; b < 256u; b++)
            for (uint32_t w = 0; w <= 256u; w++, blends++) {
                const uint32_t v = blend(a, b, w);
                if (v != (a * (256u - w) + b * w + 128u) / 256u || v > 255u || (w == 0u && v != a) || (w == 256u && v != b) || (a == b && v != a)) plain_bad++;
                // every lane of a dword with values of its own
                const uint32_t A = a | ((255u - a) << 8) | (b << 16) | (a << 24), B = b | ((255u - b) << 8) | (a << 16) | (b << 24);
                const uint32_t want = v | (blend(255u - a, 255u - b, w) << 8) | (blend(b, a, w) << 16) | (v << 24);
                if (blend_dword(A, B, w) != want) packed_bad++;
            }
    const uint32_t Ls[] = {1, 2, 5, 50, 341, 400, 1366, 65535}, ss[] = {1, 2, 3, 8, 40, 255, 256, 1000, 65535};
    for (uint32_t L : Ls)
        for (uint32_t s : ss) {
            const uint64_t M = magic(s);
            if (M != ((1ull << 40) + s - 1) / s) weight_bad++;
            for (uint32_t p = 0; p <= 256u; p++)
                for (long t = -6; t < (long) L + 6; t++, weights++) {
                    const long num = (long) p * ((long) L + (long) s) - 256 * t;
                    const uint32_t want = num <= 0 ? 0u : (num / (long) s > 256 ? 256u : (uint32_t) (num / (long) s));
                    if (weight_plain(p, L, s, t) != want || weight(p, L, s, M, (int32_t) t) != want) weight_bad++;
                }
        }
    for (uint32_t j = 0; j < 3u * 65535u + 64u; j++, thirds++)
        if (pixel_of(j) != j / 3u) third_bad++;
    for (uint32_t k = 0; k <= 17u; k++)
        if (((k * 11u) >> 5) != k / 3u) third_bad++;
    {
        Frame f = {kDissolve, 77u, 1u, 0u, 65535u, 1u, magic(1u)};
        for (long j0 = -15; j0 < 3l * 65535l; j0++, thirds++) {
            const Plan q = plan(f, j0, 0u);
            const long x = j0 >= 0 ? j0 / 3 : -((-j0 + 2) / 3), r = j0 - 3 * x;             // the floor and its remainder
            if (q.x0 != (int32_t) x || q.r != (uint32_t) r || !q.uniform || q.w != 77u || !q.from || !q.to) third_bad++;
        }
    }
    for (uint32_t k = 0; k < 3u; k++) {
        const uint32_t colour = 0x5A3C1Eu;
        const uint8_t c[3] = {0x1E, 0x3C, 0x5A};
        uint8_t got[4];
        const uint32_t word = colour_dword(colour, k);
        memcpy(got, &word, 4);
        for (uint32_t e = 0; e < 4u; e++)
            if (got[e] != c[(k + e) % 3u]) colour_bad++;
        if (colour_dword(colour | 0xFF000000u, k) != word) colour_bad++;
    }
    // frames: noise, every class of the output and of `from`, `to` a class further on; the progress and the softness walk through their ranges
    uint32_t state = 7u;
    const uint32_t Ws[] = {1, 2, 5, 6, 11, 23}, ps[] = {0, 1, 37, 128, 129, 200, 255, 256};
    for (uint32_t kind = 0; kind < (uint32_t) kKinds; kind++)
        for (uint32_t W : Ws)
            for (uint32_t lead = 0; lead < 16u; lead++)
                for (uint32_t cls = 0; cls < 16u; cls++, frames++) {
                    const uint32_t H = 3u, n = 3u * W, softness[] = {1u, 2u, W, 3u * W, 7u};
                    Frame f = {kind, ps[(lead + cls + W) % 8u], softness[(lead + 3u * cls) % 5u], 0x0AC85Au, W, H, 0u};
                    f.M = magic(f.s);
                    std::vector<uint8_t> from(n * H), to(n * H), got(n + 2);
                    for (auto& v : from) v = (uint8_t) lcg(&state);
                    for (auto& v : to) v = (uint8_t) lcg(&state);
                    bool bad = false;
                    for (uint32_t y = 0; y < H; y++) {
                        got.assign(n + 2, 0xEE);
                        blend_row(f, from.data() + y * n, to.data() + y * n, cls + y, cls + y + 1u, y, (lead + y) % 16u, got.data() + 1);
                        for (uint32_t j = 0; j < n; j++)
                            if (got[1 + j] != plain_byte(f, from[y * n + j], to[y * n + j], j / 3u, y, (int) (j % 3u))) bad = true;
                        if (got[0] != 0xEE || got[n + 1] != 0xEE) bad = true;
                    }
                    if (bad) frame_bad++;
                }
    printf("brute: blends %ld, plain mismatches %ld, packed mismatches %ld, weights %ld, weight mismatches %ld, thirds %ld, third mismatches %ld, "
           "colour mismatches %ld, frames %ld, frame mismatches %ld\n", blends, plain_bad, packed_bad, weights, weight_bad, thirds, third_bad, colour_bad, frames, frame_bad);
    return plain_bad || packed_bad || weight_bad || third_bad || colour_bad || frame_bad ? 1 : 0;
}

static bool frame_of(char** argv, Frame* f)
{
    const long W = atol(argv[0]), H = atol(argv[1]), kind = atol(argv[2]), s = atol(argv[3]);
    if (W < 1 || W > kMaxSide || H < 1 || H > kMaxSide || kind < 0 || kind >= kKinds || s < 1 || s > kMaxSoftness) return false;
    *f = Frame{(uint32_t) kind, 0u, (uint32_t) s, 0u, (uint32_t) W, (uint32_t) H, magic((uint32_t) s)};
    return true;
}

static int blend_frames(int argc, char** argv)
{
    if (argc != 12) return 2;
    char* frame_args[4] = {argv[2], argv[3], argv[5], argv[6]};
    Frame f;
    const long stride = atol(argv[4]), n = atol(argv[8]);
    if (!frame_of(frame_args, &f) || stride < 3l * f.W || n < 1) return 2;
    f.colour = (uint32_t) strtoul(argv[7], nullptr, 0);
    std::vector<uint32_t> progress;
    for (char* at = argv[9]; *at;) {
        progress.push_back((uint32_t) strtoul(at, &at, 10));
        if (*at == ',') at++;
    }
    if ((long) progress.size() != n) return 2;
    const long W = f.W, H = f.H;
    std::vector<uint8_t> in((size_t) 2 * n * H * stride), out((size_t) n * H * 3 * W);
    FILE* file = fopen(argv[10], "rb");
    if (!file || fread(in.data(), 1, in.size(), file) != in.size()) return 3;
    fclose(file);
    for (long i = 0; i < n; i++) {
        if (progress[i] > 256u) return 2;
        f.p = progress[i];
        for (long y = 0; y < H; y++) {
            const size_t from_at = ((size_t) i * H + y) * stride, to_at = ((size_t) (n + i) * H + y) * stride;
            blend_row(f, in.data() + from_at, in.data() + to_at, (uint32_t) (from_at & 15u), (uint32_t) (to_at & 15u), (uint32_t) y, (uint32_t) ((y + i) % 16),
                      out.data() + ((size_t) i * H + y) * 3 * W);
        }
    }
    file = fopen(argv[11], "wb");
    if (!file || fwrite(out.data(), 1, out.size(), file) != out.size()) return 3;
    fclose(file);
    return 0;
}

static int weights_of(int argc, char** argv)
{
    if (argc != 8) return 2;
    char* frame_args[4] = {argv[2], argv[3], argv[4], argv[5]};
    Frame f;
    if (!frame_of(frame_args, &f) || f.kind == kFade) return 2;
    f.p = (uint32_t) atol(argv[6]);
    if (f.p > 256u) return 2;
    std::vector<uint16_t> out((size_t) f.W * f.H);
    for (uint32_t y = 0; y < f.H; y++)
        for (uint32_t x = 0; x < f.W; x++) {
            const Plan q = plan(f, 3l * x, y);                               // (a piece that begins with the pixel: x0 = x)
            out[(size_t) y * f.W + x] = (uint16_t) (f.kind == kWipeLeft ? weight(f.p, f.W, f.s, f.M, (int32_t) f.W - 1 - q.x0)
                                                    : f.kind == kWipeRight ? weight(f.p, f.W, f.s, f.M, q.x0) : q.w);
        }
    FILE* file = fopen(argv[7], "wb");
    if (!file || fwrite(out.data(), 2, out.size(), file) != out.size()) return 3;
    fclose(file);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "brute")) return brute();
    if (argc >= 2 && !strcmp(argv[1], "blend")) return blend_frames(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "weights")) return weights_of(argc, argv);
    fprintf(stderr, "usage: transition_check brute | blend W H stride kind softness colour n p0,p1,... in.raw out.raw | weights W H kind softness p out.raw\n");
    return 2;
}
