// area_check.cpp -- csrc/kbe_area_block.h compiled by g++ and executed serially: the definition of kbe_area_reduce_u8 against a brute-force
// restatement (tests/test_area_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   area_check brute MAX
//       every W, H <= MAX and every w <= W, h <= H, three images each (noise, a constant, the extremes 0 and 255 in a checkerboard):
//       reduce_pixel against the restatement -- every source pixel expanded into w x h sub-cells, every target pixel the sum of its W x H
//       sub-cells, (2 S + W H) / (2 W H).  Also: the weights' sums over a target (N) and over a source (n), no weight outside span_begin ..
//       span_end, none of 0 inside, and the footprint taken in windows of every size equals the footprint taken at once.
//   area_check limits
//       the largest sides: the spans and weights of the first and last cells at N = 65535 against 64-bit arithmetic.
//   area_check reduce W H stride w h n in.raw out.raw
//       in.raw: n frames [H][stride] bytes back to back; out.raw: n frames [h][w][3].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_area_block.h"

using namespace kbe_area;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 24;
}

static int brute(int max_side)
{
    long cases = 0, pixels = 0, mismatches = 0, bad_sums = 0, bad_spans = 0, bad_windows = 0;
    uint32_t seed = 7;
    for (uint32_t N = 1; N <= (uint32_t) max_side; N++)
        for (uint32_t n = 1; n <= N; n++) {
            std::vector<uint32_t> over_targets(N, 0u);
            for (uint32_t o = 0; o < n; o++) {
                uint32_t over_sources = 0;
                for (uint32_t s = 0; s < N; s++) {
                    const uint32_t k = weight(o, s, N, n);
                    const bool inside = s >= span_begin(o, N, n) && s < span_end(o, N, n);
                    if ((k != 0u) != inside || k > n) bad_spans++;
                    over_sources += k;
                    over_targets[s] += k;
                }
                if (over_sources != N) bad_sums++;
            }
            for (uint32_t s = 0; s < N; s++)
                if (over_targets[s] != n) bad_sums++;
        }
    for (uint32_t W = 1; W <= (uint32_t) max_side; W++)
        for (uint32_t H = 1; H <= (uint32_t) max_side; H++)
            for (int kind = 0; kind < 3; kind++) {
                const size_t stride = 3 * W + (size_t) kind;                 // (rows apart by more than their pixels, too)
                std::vector<uint8_t> src(stride * H, 0xEE);
                for (uint32_t y = 0; y < H; y++)
                    for (uint32_t x = 0; x < 3 * W; x++)
                        src[y * stride + x] = kind == 0 ? (uint8_t) lcg(&seed) : kind == 1 ? (uint8_t) (W * 31 + H) : (((x / 3 + y) & 1) ? 255 : 0);
                for (uint32_t w = 1; w <= W; w++)
                    for (uint32_t h = 1; h <= H; h++) {
                        const Shape g = {W, H, w, h};
                        cases++;
                        for (uint32_t oy = 0; oy < h; oy++)
                            for (uint32_t ox = 0; ox < w; ox++) {
                                uint8_t got[3];
                                reduce_pixel(g, src.data(), stride, ox, oy, got);
                                // the restatement: the target pixel covers sub-cells [ox W, (ox + 1) W) x [oy H, (oy + 1) H); sub-cell (fx, fy) belongs to source (fx / w, fy / h)
                                uint64_t S[3] = {0, 0, 0};
                                for (uint32_t fy = oy * H; fy < (oy + 1) * H; fy++)
                                    for (uint32_t fx = ox * W; fx < (ox + 1) * W; fx++)
                                        for (int c = 0; c < 3; c++) S[c] += src[(fy / h) * stride + 3 * (fx / w) + c];
                                pixels++;
                                for (int c = 0; c < 3; c++)
                                    if (got[c] != (uint8_t) ((2 * S[c] + (uint64_t) W * H) / (2 * (uint64_t) W * H))) mismatches++;
                                // the footprint in windows of a x b sources, as a kernel takes it in strips; and from windows that cover the whole source
                                const uint32_t a = 1 + (ox + oy) % 3, b = 1 + (ox + 2 * oy) % 2;
                                uint64_t pieces[3] = {0, 0, 0}, all[3] = {0, 0, 0};
                                for (uint32_t y0 = 0; y0 < H; y0 += b)
                                    for (uint32_t x0 = 0; x0 < W; x0 += a) {
                                        const Window strip = {x0, x0 + a < W ? x0 + a : W, y0, y0 + b < H ? y0 + b : H};
                                        accumulate(g, ox, oy, intersect(footprint(g, ox, oy), strip), Rows{src.data(), stride}, pieces);
                                        accumulate(g, ox, oy, strip, Rows{src.data(), stride}, all);
                                    }
                                for (int c = 0; c < 3; c++)
                                    if (rounded(pieces[c], g) != got[c] || pieces[c] != all[c]) bad_windows++;
                            }
                    }
            }
    printf("brute: cases %ld, pixels %ld, mismatches %ld, bad sums %ld, bad spans %ld, bad windows %ld\n", cases, pixels, mismatches, bad_sums, bad_spans, bad_windows);
    return mismatches || bad_sums || bad_spans || bad_windows;
}

static int limits()
{
    long checked = 0, bad = 0;
    const uint32_t N = kMaxSide;
    for (uint32_t n : {1u, 2u, 3u, 32767u, 32768u, 65534u, 65535u})
        for (uint32_t o : {0u, 1u, n / 2, n - 2, n - 1}) {
            if (o >= n) continue;
            const uint64_t o0 = (uint64_t) o * N, o1 = o0 + N;
            const uint64_t begin = o0 / n, end = (o1 + n - 1) / n;
            if (span_begin(o, N, n) != begin || span_end(o, N, n) != end) bad++;
            uint64_t sum = 0;
            for (uint64_t s = begin > 0 ? begin - 1 : 0; s < end + 1 && s < N; s++) {
                const uint64_t s0 = s * n, s1 = s0 + n, lo = s0 > o0 ? s0 : o0, hi = s1 < o1 ? s1 : o1;
                const uint64_t want = hi > lo ? hi - lo : 0;
                if (weight(o, (uint32_t) s, N, n) != want) bad++;
                sum += want;
                checked++;
            }
            if (sum != N) bad++;
        }
    // a white 65535 x 65535 source as one pixel: S = 255 W H, the largest there is
    const Shape g = {N, N, 1u, 1u};
    if (rounded(255u * (uint64_t) N * N, g) != 255 || rounded(((uint64_t) N * N) / 2 + 1, g) != 1 || rounded(((uint64_t) N * N - 1) / 2, g) != 0) bad++;
    printf("limits: weights %ld, bad %ld\n", checked, bad);
    return bad != 0;
}

static int reduce(int argc, char** argv)
{
    if (argc != 10) return 2;
    const int W = atoi(argv[2]), H = atoi(argv[3]), stride = atoi(argv[4]), w = atoi(argv[5]), h = atoi(argv[6]), n = atoi(argv[7]);
    if (!shape_ok(W, H, w, h) || stride < 3 * W || n < 1) { fprintf(stderr, "refused\n"); return 2; }
    std::vector<uint8_t> src((size_t) n * H * stride), out((size_t) n * h * w * 3);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) { fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
    fclose(f);
    const Shape g = {(uint32_t) W, (uint32_t) H, (uint32_t) w, (uint32_t) h};
    for (int i = 0; i < n; i++)
        for (uint32_t oy = 0; oy < g.h; oy++)
            for (uint32_t ox = 0; ox < g.w; ox++)
                reduce_pixel(g, src.data() + (size_t) i * H * stride, (size_t) stride, ox, oy, &out[(((size_t) i * h + oy) * w + ox) * 3]);
    f = fopen(argv[9], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
    fclose(f);
    printf("reduced %d frames %dx%d -> %dx%d\n", n, W, H, w, h);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "brute")) return brute(atoi(argv[2]));
    if (argc == 2 && !strcmp(argv[1], "limits")) return limits();
    if (argc >= 2 && !strcmp(argv[1], "reduce")) return reduce(argc, argv);
    fprintf(stderr, "usage: area_check brute MAX | limits | reduce W H stride w h n in.raw out.raw\n");
    return 2;
}
