// crop_area_check.cpp -- csrc/kbe_crop_area_block.h compiled by g++ and executed serially: the definition of kbe_crop_area_u8 against a
// brute-force restatement (tests/test_crop_area_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   crop_area_check brute MAX
//       every W, H <= MAX, every crop cw <= W, ch <= H (so all four parities of (W - cw, H - ch), and cw == W, ch == H) and every target
//       w <= cw, h <= ch, on a frame of noise: crop_reduce_pixel against the restatement "patch, then sub-cell area sum" -- the patch
//       written out in its four forms with the border pixel repeated, every patch pixel expanded into w x h sub-cells, every target pixel
//       the sum of its cw x ch sub-cells, (2 S + cw ch) / (2 cw ch).  Also: the patch's forms against the 16-bit weighted sum
//       (sum a_ij v + 32768) >> 16 with the weights 65536 / 32768 / 16384, and start() / half() against c = N / 2 - (n - 1) / 2 in doubles.
//   crop_area_check patch W H stride cw ch n in.raw out.raw
//       the patch alone: out.raw is n frames [ch][cw][3].
//   crop_area_check reduce W H stride cw ch w h n in.raw out.raw
//       in.raw: n frames [H][stride] bytes back to back; out.raw: n frames [h][w][3].
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_crop_area_block.h"

using namespace kbe_crop_area;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 24;
}

// the patch, restated: the four forms by name, taps clamped to the frame
static uint32_t patch_restated(const uint8_t* src, size_t stride, uint32_t W, uint32_t H, uint32_t cw, uint32_t ch, uint32_t px, uint32_t py, int c)
{
    const bool half_x = (W - cw) % 2 == 0, half_y = (H - ch) % 2 == 0;
    const uint32_t x = (W - cw + 1) / 2 + px, y = (H - ch + 1) / 2 + py;
    const uint32_t xr = x + 1 < W ? x + 1 : W - 1, yb = y + 1 < H ? y + 1 : H - 1;
    const uint32_t a = src[y * stride + 3 * x + c], b = src[y * stride + 3 * xr + c], d = src[yb * stride + 3 * x + c], e = src[yb * stride + 3 * xr + c];
    if (!half_x && !half_y) return a;
    if (half_x && !half_y) return (a + b + 1) >> 1;
    if (!half_x && half_y) return (a + d + 1) >> 1;
    return (a + b + d + e + 2) >> 2;
}

static int brute(int max_side)
{
    long cases = 0, pixels = 0, mismatches = 0, bad_patches = 0, bad_weights = 0, bad_starts = 0, parities[4] = {0, 0, 0, 0};
    uint32_t seed = 11;
    for (uint32_t N = 1; N <= 64; N++)
        for (uint32_t n = 1; n <= N; n++) {
            const double c = N / 2.0 - (n - 1) / 2.0;
            if ((double) start(N, n) != floor(c) || (half(N, n) ? 0.5 : 0.0) != c - floor(c) || start(N, n) + n - 1 > N - 1 || (n < N && tap1(N, n, n - 1) != start(N, n) + n - 1 + (half(N, n) ? 1 : 0))) bad_starts++;
        }
    for (uint32_t W = 1; W <= (uint32_t) max_side; W++)
        for (uint32_t H = 1; H <= (uint32_t) max_side; H++) {
            const size_t stride = 3 * W + (W + H) % 3;                       // (rows apart by more than their pixels, too)
            std::vector<uint8_t> src(stride * H, 0xEE);
            for (uint32_t y = 0; y < H; y++)
                for (uint32_t x = 0; x < 3 * W; x++) src[y * stride + x] = (uint8_t) lcg(&seed);
            for (uint32_t cw = 1; cw <= W; cw++)
                for (uint32_t ch = 1; ch <= H; ch++) {
                    const Crop k = {W, H, cw, ch};
                    const Patch patch = {src.data(), stride, k};
                    parities[2 * ((W - cw) & 1) + ((H - ch) & 1)]++;
                    // the patch: the header's one form against the four by name, and against the 16-bit weighted sum of the kernel of kbe_hip.hip
                    std::vector<uint8_t> p((size_t) cw * ch * 3);
                    const uint32_t fx = half(W, cw) ? 32768u : 0u, fy = half(H, ch) ? 32768u : 0u;             // the fractions, in 1 / 65536
                    const uint64_t a11 = (uint64_t) (65536u - fx) * (65536u - fy) >> 16, a12 = (uint64_t) fx * (65536u - fy) >> 16, a21 = (uint64_t) (65536u - fx) * fy >> 16, a22 = (uint64_t) fx * fy >> 16;
                    for (uint32_t py = 0; py < ch; py++)
                        for (uint32_t px = 0; px < cw; px++)
                            for (int c = 0; c < 3; c++) {
                                const uint32_t v = patch.row(py)(px, c);
                                p[((size_t) py * cw + px) * 3 + c] = (uint8_t) v;
                                if (v != patch_restated(src.data(), stride, W, H, cw, ch, px, py, c) || v > 255u) bad_patches++;
                                const uint32_t x0 = tap0(W, cw, px), x1 = tap1(W, cw, px), y0 = tap0(H, ch, py), y1 = tap1(H, ch, py);
                                const uint64_t sum = a11 * src[y0 * stride + 3 * x0 + c] + a12 * src[y0 * stride + 3 * x1 + c] + a21 * src[y1 * stride + 3 * x0 + c] + a22 * src[y1 * stride + 3 * x1 + c];
                                if (v != (uint32_t) ((sum + 32768u) >> 16)) bad_weights++;
                            }
                    if (whole(k) != (fx == 0u && fy == 0u)) bad_patches++;
                    for (uint32_t w = 1; w <= cw; w++)
                        for (uint32_t h = 1; h <= ch; h++) {
                            cases++;
                            for (uint32_t oy = 0; oy < h; oy++)
                                for (uint32_t ox = 0; ox < w; ox++) {
                                    uint8_t got[3];
                                    crop_reduce_pixel(k, w, h, src.data(), stride, ox, oy, got);
                                    // the target pixel covers sub-cells [ox cw, (ox + 1) cw) x [oy ch, (oy + 1) ch); sub-cell (fx, fy) belongs to patch pixel (fx / w, fy / h)
                                    uint64_t S[3] = {0, 0, 0};
                                    for (uint32_t sy = oy * ch; sy < (oy + 1) * ch; sy++)
                                        for (uint32_t sx = ox * cw; sx < (ox + 1) * cw; sx++)
                                            for (int c = 0; c < 3; c++) S[c] += p[((size_t) (sy / h) * cw + sx / w) * 3 + c];
                                    pixels++;
                                    for (int c = 0; c < 3; c++)
                                        if (got[c] != (uint8_t) ((2 * S[c] + (uint64_t) cw * ch) / (2 * (uint64_t) cw * ch))) mismatches++;
                                }
                        }
                }
        }
    printf("brute: cases %ld, pixels %ld, mismatches %ld, bad patches %ld, bad weights %ld, bad starts %ld, parities %ld %ld %ld %ld\n", cases, pixels, mismatches, bad_patches,
           bad_weights, bad_starts, parities[0], parities[1], parities[2], parities[3]);
    return mismatches || bad_patches || bad_weights || bad_starts;
}

static bool read_frames(const char* path, std::vector<uint8_t>& src)
{
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(src.data(), 1, src.size(), f) == src.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

static bool write_frames(const char* path, const std::vector<uint8_t>& out)
{
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot write %s\n", path);
    return ok;
}

// `reduce`, or with patch_only the patch itself (w = cw, h = ch are not reduced: read through Patch, no area arithmetic at all)
static int run(char** argv, bool patch_only)
{
    const int W = atoi(argv[2]), H = atoi(argv[3]), stride = atoi(argv[4]), cw = atoi(argv[5]), ch = atoi(argv[6]);
    const int w = patch_only ? cw : atoi(argv[7]), h = patch_only ? ch : atoi(argv[8]), n = atoi(argv[patch_only ? 7 : 9]);
    if (!shape_ok(W, H, cw, ch, w, h) || stride < 3 * W || n < 1) { fprintf(stderr, "refused\n"); return 2; }
    std::vector<uint8_t> src((size_t) n * H * stride), out((size_t) n * h * w * 3);
    if (!read_frames(argv[patch_only ? 8 : 10], src)) return 2;
    const Crop k = {(uint32_t) W, (uint32_t) H, (uint32_t) cw, (uint32_t) ch};
    for (int i = 0; i < n; i++) {
        const uint8_t* frame = src.data() + (size_t) i * H * stride;
        for (uint32_t oy = 0; oy < (uint32_t) h; oy++)
            for (uint32_t ox = 0; ox < (uint32_t) w; ox++) {
                uint8_t* to = &out[(((size_t) i * h + oy) * w + ox) * 3];
                if (patch_only)
                    for (int c = 0; c < 3; c++) to[c] = (uint8_t) Patch{frame, (size_t) stride, k}.row(oy)(ox, c);
                else crop_reduce_pixel(k, (uint32_t) w, (uint32_t) h, frame, (size_t) stride, ox, oy, to);
            }
    }
    if (!write_frames(argv[patch_only ? 9 : 11], out)) return 2;
    printf("%s %d frames %dx%d, crop %dx%d -> %dx%d\n", patch_only ? "patch of" : "reduced", n, W, H, cw, ch, w, h);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "brute")) return brute(atoi(argv[2]));
    if (argc == 10 && !strcmp(argv[1], "patch")) return run(argv, true);
    if (argc == 12 && !strcmp(argv[1], "reduce")) return run(argv, false);
    fprintf(stderr, "usage: crop_area_check brute MAX | patch W H stride cw ch n in.raw out.raw | reduce W H stride cw ch w h n in.raw out.raw\n");
    return 2;
}
