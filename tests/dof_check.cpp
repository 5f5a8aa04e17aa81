// dof_check.cpp -- csrc/kbe_dof_block.h compiled by g++ and executed serially: the definition of kbe_dof_u8 against a restatement that
// scatters (tests/test_dof_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   dof_check brute
//       the table: n(e) against the list written out below, kWeight[e] = 8192 / n(e), and the 32-bit bound of the sums from the table;
//       every W, H <= 7, R in {0, 1, 2, 3}, noise frames, depths drawn from five levels, three apertures: gather_pixel against the
//       restatement "for every q, visit the disc of its radius, apply the occlusion rule from the target's side", accumulated in 64 bits;
//       one 40 x 24 case at R = 16 the same way.
//   dof_check radius zf A R n in.f32 out.u8
//       radius() of n depths.
//   dof_check blur W H stride z_stride R A n in.raw depth.f32 focus.f32 out.raw
//       in.raw: n frames [H][stride] bytes back to back; depth.f32: n planes [H][z_stride] floats; focus.f32: n floats; out.raw: n frames
//       [H][W][3].  A is decimal text that strtof reads back exactly (9 significant digits).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_dof_block.h"

using namespace kbe_dof;

static const uint32_t kDisc[kMaxRadius + 1] = {1, 5, 13, 29, 49, 81, 113, 149, 197, 253, 317, 377, 441, 529, 613, 709, 797};
static const uint32_t kListed[kMaxRadius + 1] = {8192, 1638, 630, 282, 167, 101, 72, 54, 41, 32, 25, 21, 18, 15, 13, 11, 10};

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 24;
}

static void radii(const float* z, size_t z_stride, uint32_t W, uint32_t H, float zf, float A, int R, std::vector<uint8_t>& r)
{
    r.resize((size_t) W * H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) r[(size_t) y * W + x] = (uint8_t) radius(z[(size_t) y * z_stride + x], zf, A, R);
}

// the restatement: every sample q spreads over the disc of its own radius; what it adds to a target p is decided from p's side
static long scattered(uint32_t W, uint32_t H, const uint8_t* src, size_t stride, const float* z, size_t z_stride, const std::vector<uint8_t>& r, const uint8_t* got)
{
    std::vector<uint64_t> sums((size_t) W * H * 4, 0);
    for (long qy = 0; qy < (long) H; qy++)
        for (long qx = 0; qx < (long) W; qx++) {
            const long rq = r[qy * W + qx];
            for (long py = qy - rq; py <= qy + rq; py++)
                for (long px = qx - rq; px <= qx + rq; px++) {
                    if (px < 0 || py < 0 || px >= (long) W || py >= (long) H) continue;
                    const long d2 = (px - qx) * (px - qx) + (py - qy) * (py - qy), rp = r[py * W + px];
                    long e = rq;
                    if (!(z[qy * z_stride + qx] <= z[py * z_stride + px])) e = rq < rp ? rq : rp;
                    if (d2 > e * e) continue;
                    const uint64_t w = 8192u / kDisc[e];
                    uint64_t* s = &sums[(size_t) (py * W + px) * 4];
                    s[3] += w;
                    for (int c = 0; c < 3; c++) s[c] += w * src[qy * stride + 3 * qx + c];
                }
        }
    long bad = 0;
    for (size_t i = 0; i < (size_t) W * H; i++)
        for (int c = 0; c < 3; c++) bad += got[3 * i + c] != (uint8_t) ((2 * sums[4 * i + c] + sums[4 * i + 3]) / (2 * sums[4 * i + 3]));
    return bad;
}

static long one_case(uint32_t W, uint32_t H, int R, float A, float zf, uint32_t* seed, long* blurred)
{
    static const float levels[5] = {50.0f, 80.0f, 100.0f, 160.0f, 400.0f};
    const size_t stride = 3 * W + (W + H) % 3, z_stride = W + (W * H) % 2;
    std::vector<uint8_t> src(stride * H, 0xEE), got((size_t) W * H * 3), r;
    std::vector<float> z(z_stride * H, -1.0f);
    for (uint32_t y = 0; y < H; y++) {
        for (uint32_t x = 0; x < 3 * W; x++) src[y * stride + x] = (uint8_t) lcg(seed);
        for (uint32_t x = 0; x < W; x++) z[y * z_stride + x] = levels[lcg(seed) % 5u];
    }
    radii(z.data(), z_stride, W, H, zf, A, R, r);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            gather_pixel(W, H, src.data(), stride, z.data(), z_stride, r.data(), R, x, y, &got[((size_t) y * W + x) * 3]);
            *blurred += r[(size_t) y * W + x] > 0;
        }
    return scattered(W, H, src.data(), stride, z.data(), z_stride, r, got.data());
}

static int brute()
{
    long bad_table = 0, mismatches = 0, cases = 0, blurred = 0;
    for (int e = 0; e <= kMaxRadius; e++) bad_table += disc_points(e) != kDisc[e] || kWeight.w[e] != 8192u / kDisc[e] || kWeight.w[e] != kListed[e];
    // the 32-bit bound: the target itself at weight kWeight[0], every other cell of the 33 x 33 window at the largest weight a sample at d > 0 can have
    uint64_t largest = 0;
    for (int e = 1; e <= kMaxRadius; e++) largest = kWeight.w[e] > largest ? kWeight.w[e] : largest;
    const uint64_t taps = (uint64_t) (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1) - 1, sum_w = kWeight.w[0] + taps * largest, sum_wv = 255u * sum_w;
    const bool fits = largest == 1638u && taps == 1088u && sum_wv == 456535680ull && 2 * sum_wv + sum_w < (1ull << 32);
    uint32_t seed = 7;
    for (uint32_t W = 1; W <= 7; W++)
        for (uint32_t H = 1; H <= 7; H++)
            for (int R = 0; R <= 3; R++)
                for (float A : {0.8f, 2.5f, 6.0f}) {
                    mismatches += one_case(W, H, R, A, 100.0f, &seed, &blurred);
                    cases++;
                }
    mismatches += one_case(40, 24, 16, 22.0f, 80.0f, &seed, &blurred);
    cases++;
    printf("brute: cases %ld, blurred pixels %ld, mismatches %ld, bad table entries %ld, sums fit 32 bits: %s (2 sum(wv) + sum(w) <= %llu)\n", cases, blurred, mismatches, bad_table,
           fits ? "yes" : "NO", (unsigned long long) (2 * sum_wv + sum_w));
    return mismatches || bad_table || !fits || !blurred;
}

template <class T>
static bool read_file(const char* path, std::vector<T>& to)
{
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(to.data(), sizeof(T), to.size(), f) == to.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

static bool write_file(const char* path, const std::vector<uint8_t>& out)
{
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot write %s\n", path);
    return ok;
}

static int run_radius(char** argv)
{
    const float zf = strtof(argv[2], nullptr), A = strtof(argv[3], nullptr);
    const int R = atoi(argv[4]), n = atoi(argv[5]);
    if (n < 1 || R < 0 || R > kMaxRadius) { fprintf(stderr, "refused\n"); return 2; }
    std::vector<float> z((size_t) n);
    std::vector<uint8_t> out((size_t) n);
    if (!read_file(argv[6], z)) return 2;
    for (int i = 0; i < n; i++) out[i] = (uint8_t) radius(z[i], zf, A, R);
    return write_file(argv[7], out) ? 0 : 2;
}

static int run_blur(char** argv)
{
    const int W = atoi(argv[2]), H = atoi(argv[3]), stride = atoi(argv[4]), z_stride = atoi(argv[5]), R = atoi(argv[6]), n = atoi(argv[8]);
    const float A = strtof(argv[7], nullptr);
    if (!shape_ok(W, H, R) || stride < 3 * W || z_stride < W || n < 1 || !(A >= 0.0f)) { fprintf(stderr, "refused\n"); return 2; }
    std::vector<uint8_t> src((size_t) n * H * stride), out((size_t) n * H * W * 3), r;
    std::vector<float> z((size_t) n * H * z_stride), focus((size_t) n);
    if (!read_file(argv[9], src) || !read_file(argv[10], z) || !read_file(argv[11], focus)) return 2;
    for (int i = 0; i < n; i++) {
        const uint8_t* frame = src.data() + (size_t) i * H * stride;
        const float* plane = z.data() + (size_t) i * H * z_stride;
        radii(plane, (size_t) z_stride, (uint32_t) W, (uint32_t) H, focus[i], A, R, r);
        for (uint32_t y = 0; y < (uint32_t) H; y++)
            for (uint32_t x = 0; x < (uint32_t) W; x++)
                gather_pixel((uint32_t) W, (uint32_t) H, frame, (size_t) stride, plane, (size_t) z_stride, r.data(), R, x, y, &out[(((size_t) i * H + y) * W + x) * 3]);
    }
    if (!write_file(argv[12], out)) return 2;
    printf("blurred %d frames %dx%d, R %d\n", n, W, H, R);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "brute")) return brute();
    if (argc == 8 && !strcmp(argv[1], "radius")) return run_radius(argv);
    if (argc == 13 && !strcmp(argv[1], "blur")) return run_blur(argv);
    fprintf(stderr, "usage: dof_check brute | radius zf A R n in.f32 out.u8 | blur W H stride z_stride R A n in.raw depth.f32 focus.f32 out.raw\n");
    return 2;
}
