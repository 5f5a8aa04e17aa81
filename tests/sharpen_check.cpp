// sharpen_check.cpp -- csrc/kbe_sharpen_block.h compiled by g++ and executed serially: the definition of kbe_sharpen_u8
// (tests/test_sharpen_stream.py).  Build: g++ -O2 -std=c++17 -fsanitize=signed-integer-overflow,address -fno-sanitize-recover=all -I csrc
// (no -ffast-math, no -march); a plain program, run as it is.
//
//   sharpen_check brute
//       every R in 1..24, seeded taps that add up to 32768, small seeded frames (1x1, 5x3, 3x7, 9x8: every tap clamped at the larger R),
//       seeded amounts and thresholds and the extremes of both: sharpen_pixel() against the four formulas of include/kbe_sharpen.h
//       evaluated by brute force in __int128, a floor computed by comparison and not by a shift.
//   sharpen_check limits
//       the worst cases of the 32-bit bounds, the same way, under the sanitizer: all-255 and all-0 frames and a 0 / 255 checkerboard at
//       amount 1024 and amount 1, every R, with all the weight on the centre tap, on the outermost pair of taps, and spread evenly; reports
//       the largest sums seen against the bounds the header states.
//   sharpen_check sharpen W H stride n amount threshold R w0 .. wR in.raw out.raw
//       in.raw: n frames [H][stride] bytes back to back; out.raw: n frames [H][W][3].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_sharpen_block.h"

using namespace kbe_sharpen;
typedef __int128 wide;

struct Tally {
    long cases = 0, bytes = 0, bad = 0, negative = 0, bad_floors = 0, clamped_low = 0, clamped_high = 0, kept = 0;
    long long row_max = 0, column_max = 0, gain_max = 0;
};

// floor(a / 2^bits) without a shift of a negative value
static wide floor_shift(wide a, int bits)
{
    const wide one = (wide) 1 << bits;
    wide q = a / one;
    if (a - q * one < 0) q -= 1;
    return q;
}

static wide at(const uint8_t* src, size_t stride, int W, int H, int x, int y, int c)
{
    x = x < 0 ? 0 : x > W - 1 ? W - 1 : x;
    y = y < 0 ? 0 : y > H - 1 ? H - 1 : y;
    return src[(size_t) y * stride + 3 * (size_t) x + c];
}

static void check_frame(const Taps& t, int amount, int threshold, const uint8_t* src, size_t stride, int W, int H, Tally& tally)
{
    tally.cases++;
    const int R = t.radius;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            uint8_t got[3];
            sharpen_pixel(t, amount, threshold, src, stride, (uint32_t) W, (uint32_t) H, (uint32_t) x, (uint32_t) y, got);
            for (int c = 0; c < 3; c++) {
                wide column = 0;
                for (int j = -R; j <= R; j++) {
                    wide row = 0;
                    for (int k = -R; k <= R; k++) row += (wide) t.w[k < 0 ? -k : k] * at(src, stride, W, H, x + k, y + j, c);
                    if (row + 64 > tally.row_max) tally.row_max = (long long) (row + 64);
                    column += (wide) t.w[j < 0 ? -j : j] * floor_shift(row + 64, 7);
                }
                if (column + 16384 > tally.column_max) tally.column_max = (long long) (column + 16384);
                const wide v = at(src, stride, W, H, x, y, c), b16 = floor_shift(column + 16384, 15), d = 256 * v - b16;
                wide want = v;
                if (!((d < 0 ? -d : d) < 256 * (wide) threshold)) {
                    const wide product = (wide) amount * d;
                    const wide magnitude = (product < 0 ? -product : product) + 32768;
                    if (magnitude > tally.gain_max) tally.gain_max = (long long) magnitude;
                    const wide step = floor_shift(product + 32768, 16);
                    if (product < 0) {
                        tally.negative++;
                        // the compiler's shift of this negative value, as the header writes it, must be the floor
                        if ((wide) (((int32_t) product + 32768) >> 16) != step) tally.bad_floors++;
                    }
                    want = v + step;
                    if (want < 0) { want = 0; tally.clamped_low++; }
                    if (want > 255) { want = 255; tally.clamped_high++; }
                } else
                    tally.kept++;
                tally.bytes++;
                if ((wide) got[c] != want) tally.bad++;
            }
        }
}

static uint32_t g_seed = 12345u;
static uint32_t rnd()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

// seeded taps of radius R that add up to kOne: the outer ones at random below an even share, the centre by difference
static Taps random_taps(int R)
{
    Taps t = {};
    t.radius = R;
    uint32_t outer = 0;
    for (int k = 1; k <= R; k++) {
        t.w[k] = rnd() % (uint32_t) (kOne / (2 * R) + 1);
        outer += t.w[k];
    }
    t.w[0] = (uint32_t) kOne - 2u * outer;
    return t;
}

static int report(const char* what, const Tally& t)
{
    printf("%s: cases %ld, bytes %ld, bad %ld, negative %ld, bad floors %ld, clamped low %ld, clamped high %ld, kept %ld, row max %lld, column max %lld, gain max %lld\n", what, t.cases,
           t.bytes, t.bad, t.negative, t.bad_floors, t.clamped_low, t.clamped_high, t.kept, t.row_max, t.column_max, t.gain_max);
    return t.bad || t.bad_floors;
}

static int brute()
{
    Tally tally;
    const int sizes[4][2] = {{1, 1}, {5, 3}, {3, 7}, {9, 8}};
    for (int R = 1; R <= kMaxRadius; R++)
        for (int s = 0; s < 4; s++) {
            const int W = sizes[s][0], H = sizes[s][1];
            const size_t stride = 3 * (size_t) W + (size_t) (s % 3);
            std::vector<uint8_t> frame(stride * H);
            for (int round = 0; round < 3; round++) {
                for (uint8_t& b : frame) b = round == 2 ? (uint8_t) ((rnd() & 1u) * 255u) : (uint8_t) rnd();
                const Taps t = random_taps(R);
                const int amount = round == 0 ? 1 + (int) (rnd() % 1024u) : round == 1 ? 1024 : 1, threshold = round == 0 ? (int) (rnd() % 8u) : round == 1 ? 0 : 255;
                check_frame(t, amount, threshold, frame.data(), stride, W, H, tally);
            }
        }
    return report("brute", tally);
}

static int limits()
{
    Tally tally;
    const int W = 6, H = 5;
    std::vector<uint8_t> frame(3 * (size_t) W * H);
    for (int R = 1; R <= kMaxRadius; R++)
        for (int shape = 0; shape < 3; shape++) {
            Taps t = {};
            t.radius = R;
            if (shape == 0) t.w[0] = kOne;                                    // all the weight on the centre
            else if (shape == 1) t.w[R] = kOne / 2;                           // ... on the outermost pair
            else {                                                            // ... spread evenly
                for (int k = 1; k <= R; k++) t.w[k] = (uint32_t) (kOne / (2 * R + 1));
                t.w[0] = (uint32_t) kOne - 2u * (uint32_t) R * t.w[1];
            }
            uint32_t sum = t.w[0];
            for (int k = 1; k <= R; k++) sum += 2u * t.w[k];
            if (sum != (uint32_t) kOne) return 3;
            for (int picture = 0; picture < 3; picture++) {
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++)
                        for (int c = 0; c < 3; c++) frame[((size_t) y * W + x) * 3 + c] = picture == 0 ? 255 : picture == 1 ? 0 : (uint8_t) (((x + y) & 1) * 255);
                for (int amount : {1024, 1})
                    for (int threshold : {0, 255}) check_frame(t, amount, threshold, frame.data(), 3 * (size_t) W, W, H, tally);
            }
        }
    return report("limits", tally);
}

static int run(int argc, char** argv)
{
    const int W = atoi(argv[2]), H = atoi(argv[3]), stride = atoi(argv[4]), n = atoi(argv[5]), amount = atoi(argv[6]), threshold = atoi(argv[7]), R = atoi(argv[8]);
    if (!(R >= 1 && R <= kMaxRadius) || argc != 9 + R + 1 + 2) { fprintf(stderr, "refused: radius\n"); return 2; }
    uint16_t given[kMaxRadius + 1];
    Taps t = {};
    t.radius = R;
    for (int k = 0; k <= R; k++) t.w[k] = given[k] = (uint16_t) atoi(argv[9 + k]);
    if (!shape_ok(W, H, amount, threshold) || !taps_ok(given, R) || stride < 3 * W || n < 1) { fprintf(stderr, "refused\n"); return 2; }
    const char* const in = argv[9 + R + 1];
    const char* const to = argv[9 + R + 2];
    std::vector<uint8_t> src((size_t) n * H * stride), out((size_t) n * H * W * 3);
    FILE* f = fopen(in, "rb");
    const bool read = f && fread(src.data(), 1, src.size(), f) == src.size();
    if (f) fclose(f);
    if (!read) { fprintf(stderr, "cannot read %s\n", in); return 2; }
    for (int i = 0; i < n; i++)
        for (uint32_t y = 0; y < (uint32_t) H; y++)
            for (uint32_t x = 0; x < (uint32_t) W; x++)
                sharpen_pixel(t, amount, threshold, src.data() + (size_t) i * H * stride, (size_t) stride, (uint32_t) W, (uint32_t) H, x, y, &out[(((size_t) i * H + y) * W + x) * 3]);
    f = fopen(to, "wb");
    const bool written = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if (f) fclose(f);
    if (!written) { fprintf(stderr, "cannot write %s\n", to); return 2; }
    printf("sharpened %d frames %dx%d, radius %d, amount %d, threshold %d\n", n, W, H, R, amount, threshold);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "brute")) return brute();
    if (argc == 2 && !strcmp(argv[1], "limits")) return limits();
    if (argc >= 13 && !strcmp(argv[1], "sharpen")) return run(argc, argv);
    fprintf(stderr, "usage: sharpen_check brute | limits | sharpen W H stride n amount threshold R w0 .. wR in.raw out.raw\n");
    return 2;
}
