// grade_check.cpp -- csrc/kbe_grade_block.h compiled by g++ and executed serially: the packed forms the kernel of kbe_grade_u8 computes with,
// held to the plain definition (tests/test_grade_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   grade_check brute N
//       a seeded random table of N nodes per axis and all 2^24 colours: grade_pixel against the plain form (cell_plain, a stable sort,
//       tetra_plain with its / 255) byte for byte; wherever two fractions are equal, all six orders of looking at the axes against each
//       other; every result against the float interpolation of the same nodes within 0.5 (+ 1e-9).
//   grade_check forms
//       cell against cell_plain and the division without a divide against / 255 for every N in 2..33 and every byte; mix_pixel against
//       mix_plain in every lane for all 256 x 256 x 257 (c, g, s), s = 256 giving g and s = 0 giving c; unpack_run / pack_run and
//       run_from_aligned / run_to_aligned against the bytes; whole rows (grade_row) at all four classes of their address and widths from 1
//       pixel on, against the plain form pixel by pixel, the bytes around the row untouched.
//   grade_check identity
//       the identity table with nodes round(255 j / (N - 1)) for every N in 2..33: on every colour of a lattice (each channel through all
//       256 values against 24 values of the two others) within 1, and exact where (N - 1) | 255; for N = 2, 4, 6, 16, 18 exact on all
//       2^24 colours.
//   grade_check grade W H stride n N s0,s1,... in.raw out.raw
//       in.raw: the n frames, [H][stride] bytes each, back to back, then the table's N^3 dwords; out.raw: the n frames as they are afterwards,
//       padding included.  A row is taken at the class of its first byte's offset in the file.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_grade_block.h"

using namespace kbe_grade;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 8;
}

static std::vector<uint32_t> random_table(uint32_t N, uint32_t seed)
{
    std::vector<uint32_t> lut(N * N * N);
    uint32_t state = seed;
    for (auto& v : lut) v = (lcg(&state) & 0xFFFFFFu) | (lcg(&state) << 24);           // (byte 3: noise, ignored)
    return lut;
}

static std::vector<uint32_t> identity_table(uint32_t N)
{
    std::vector<uint32_t> lut(N * N * N);
    std::vector<uint32_t> node(N);
    for (uint32_t j = 0; j < N; j++) node[j] = (2u * 255u * j + (N - 1u)) / (2u * (N - 1u));       // round(255 j / (N - 1))
    for (uint32_t i2 = 0; i2 < N; i2++)
        for (uint32_t i1 = 0; i1 < N; i1++)
            for (uint32_t i0 = 0; i0 < N; i0++) lut[(i2 * N + i1) * N + i0] = node[i0] | (node[i1] << 8) | (node[i2] << 16) | 0xAB000000u;
    return lut;
}

// the same interpolation in double, of the same nodes, unrounded
static void tetra_float(uint32_t x, const uint32_t* lut, uint32_t N, double out[3])
{
    uint32_t i[3], f[3];
    for (int k = 0; k < 3; k++) cell_plain((x >> (8 * k)) & 255u, N, &i[k], &f[k]);
    int axis[3] = {0, 1, 2};
    for (int a = 1; a < 3; a++)
        for (int b = a; b > 0 && f[axis[b]] > f[axis[b - 1]]; b--) {
            const int t = axis[b];
            axis[b] = axis[b - 1], axis[b - 1] = t;
        }
    const uint32_t step[3] = {1u, N, N * N}, base = (i[2] * N + i[1]) * N + i[0];
    const uint32_t v[4] = {lut[base], lut[base + step[axis[0]]], lut[base + step[axis[0]] + step[axis[1]]], lut[base + 1u + N + N * N]};
    const double w[4] = {(255.0 - f[axis[0]]) / 255.0, ((double) f[axis[0]] - f[axis[1]]) / 255.0, ((double) f[axis[1]] - f[axis[2]]) / 255.0, f[axis[2]] / 255.0};
    for (int k = 0; k < 3; k++) {
        out[k] = 0.0;
        for (int j = 0; j < 4; j++) out[k] += w[j] * ((v[j] >> (8 * k)) & 255u);
    }
}

static int brute(uint32_t N)
{
    if (N < (uint32_t) kMinNodes || N > (uint32_t) kMaxNodes) return 2;
    const std::vector<uint32_t> lut = random_table(N, 1000u + N);
    long colours = 0, packed_bad = 0, ties = 0, tie_bad = 0, float_bad = 0, range_bad = 0;
    for (uint32_t x = 0; x < (1u << 24); x++, colours++) {
        const uint32_t got = grade_pixel(x | 0x5A000000u, lut.data(), N), want = grade_plain(x, lut.data(), N, 0);
        if (got != want) packed_bad++;
        if (got >> 24) range_bad++;
        uint32_t i[3], f[3];
        for (int k = 0; k < 3; k++) {
            cell_plain((x >> (8 * k)) & 255u, N, &i[k], &f[k]);
            if (i[k] > N - 2u || f[k] > 255u) range_bad++;
        }
        if (f[0] == f[1] || f[1] == f[2] || f[0] == f[2]) {
            ties++;
            for (int order = 1; order < 6; order++)
                if (grade_plain(x, lut.data(), N, order) != want) tie_bad++;
        }
        double exact[3];
        tetra_float(x, lut.data(), N, exact);
        for (int k = 0; k < 3; k++)
            if (fabs((double) ((want >> (8 * k)) & 255u) - exact[k]) > 0.5 + 1e-9) float_bad++;
    }
    printf("brute: N %u, colours %ld, packed mismatches %ld, ties %ld, tie mismatches %ld, float mismatches %ld, range mismatches %ld\n", N, colours, packed_bad, ties, tie_bad,
           float_bad, range_bad);
    return packed_bad || tie_bad || float_bad || range_bad ? 1 : 0;
}

static int forms()
{
    long cells = 0, cell_bad = 0, mixes = 0, mix_bad = 0, run_bad = 0, rows = 0, row_bad = 0;
    for (uint32_t N = kMinNodes; N <= (uint32_t) kMaxNodes; N++)
        for (uint32_t v = 0; v < 256u; v++, cells++) {
            uint32_t i, f, pi, pf;
            cell(v, N, &i, &f);
            cell_plain(v, N, &pi, &pf);
            const uint32_t p = v * (N - 1u);
            if (i != pi || f != pf || div255(p + 1u) != p / 255u || div255_mul(p) != p / 255u || i > N - 2u || f > 255u || 255u * i + f != p || (f == 255u) != (v == 255u)) cell_bad++;
        }
    for (uint32_t n = 0; n <= 65152u; n++)
        if (div255(n + 1u) != n / 255u) cell_bad++;
    for (uint32_t n = 0; n < 65536u; n++)
        if (div255_mul(n) != n / 255u) cell_bad++;
    for (uint32_t c = 0; c < 256u; c++)
        for (uint32_t g = 0; g < 256u; g++)
            for (uint32_t s = 0; s <= 256u; s++, mixes++) {
                const uint32_t want = mix_plain(c, g, s);
                if (want > 255u || (s == 256u && want != g) || (s == 0u && want != c) || (c == g && want != c)) mix_bad++;
                // every lane with values of its own
                const uint32_t C = c | ((255u - c) << 8) | (g << 16) | 0x77000000u, G = g | ((255u - g) << 8) | (c << 16) | 0x99000000u;
                if (mix_pixel(C, G, s) != (want | (mix_plain(255u - c, 255u - g, s) << 8) | (mix_plain(g, c, s) << 16))) mix_bad++;
            }
    {
        uint8_t bytes[52], back[52];
        uint32_t c[kRunDwords], px[kRunPixels], again[kRunDwords], x[kRunDwords + 1];
        for (int i = 0; i < 52; i++) bytes[i] = (uint8_t) (3 * i + 1);
        memcpy(c, bytes, kRunBytes);
        unpack_run(c, px);
        for (int k = 0; k < kRunPixels; k++)
            if (px[k] != ((uint32_t) bytes[3 * k] | ((uint32_t) bytes[3 * k + 1] << 8) | ((uint32_t) bytes[3 * k + 2] << 16))) run_bad++;
        pack_run(px, again);
        if (memcmp(again, c, sizeof(c))) run_bad++;
        for (uint32_t b = 1; b < 4u; b++) {
            memcpy(x, bytes, 52);
            run_from_aligned(x, b, c);
            if (memcmp(c, bytes + b, kRunBytes)) run_bad++;
            run_to_aligned(c, b, x);
            memcpy(back, x, 52);
            for (uint32_t i = 0; i < 52u; i++)
                if (back[i] != (i >= b && i < b + (uint32_t) kRunBytes ? bytes[i] : 0)) run_bad++;
        }
    }
    // rows: noise, every class of the row's address; the strength and the table's size walk through their ranges
    uint32_t state = 11u;
    const int32_t widths[] = {1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 40, 100};
    const uint32_t strengths[] = {1, 37, 128, 129, 200, 255, 256};
    const uint32_t sizes[] = {2, 3, 5, 9, 17, 25, 32, 33};
    for (int32_t pixels : widths)
        for (uint32_t lead = 0; lead < 4u; lead++)
            for (uint32_t t = 0; t < 8u; t++, rows++) {
                const uint32_t N = sizes[t], s = strengths[(lead + t + (uint32_t) pixels) % 7u];
                const std::vector<uint32_t> lut = random_table(N, 77u + t);
                std::vector<uint8_t> row(3 * pixels + 2), before;
                for (auto& v : row) v = (uint8_t) lcg(&state);
                if (pixels > 2) row[1] = row[2] = row[3] = 255, row[4] = row[5] = row[6] = 0;
                before = row;
                grade_row(row.data() + 1, pixels, lut.data(), N, s, lead);
                bool bad = row[0] != before[0] || row[3 * pixels + 1] != before[3 * pixels + 1];
                for (int32_t k = 0; k < pixels; k++) {
                    const uint32_t x = (uint32_t) before[1 + 3 * k] | ((uint32_t) before[2 + 3 * k] << 8) | ((uint32_t) before[3 + 3 * k] << 16), g = grade_plain(x, lut.data(), N, (int) (t % 6u));
                    for (int ch = 0; ch < 3; ch++)
                        if (row[1 + 3 * k + ch] != mix_plain((x >> (8 * ch)) & 255u, (g >> (8 * ch)) & 255u, s)) bad = true;
                }
                if (bad) row_bad++;
            }
    printf("forms: cells %ld, cell mismatches %ld, mixes %ld, mix mismatches %ld, run mismatches %ld, rows %ld, row mismatches %ld\n", cells, cell_bad, mixes, mix_bad, run_bad, rows, row_bad);
    return cell_bad || mix_bad || run_bad || row_bad ? 1 : 0;
}

static int identity()
{
    long lattice = 0, within_bad = 0, exact_sizes = 0, exact_bad = 0, full = 0, full_bad = 0;
    uint32_t others[24];
    for (uint32_t k = 0; k < 24u; k++) others[k] = k == 23u ? 255u : 11u * k + (k & 1u);
    for (uint32_t N = kMinNodes; N <= (uint32_t) kMaxNodes; N++) {
        const std::vector<uint32_t> lut = identity_table(N);
        const bool exact = 255u % (N - 1u) == 0u;
        exact_sizes += exact ? 1 : 0;
        for (int ch = 0; ch < 3; ch++)
            for (uint32_t v = 0; v < 256u; v++)
                for (uint32_t a = 0; a < 24u; a++)
                    for (uint32_t b = 0; b < 24u; b++, lattice++) {
                        const uint32_t x = (v << (8 * ch)) | (others[a] << (8 * ((ch + 1) % 3))) | (others[b] << (8 * ((ch + 2) % 3))), g = grade_pixel(x, lut.data(), N);
                        for (int k = 0; k < 3; k++) {
                            const int off = (int) ((g >> (8 * k)) & 255u) - (int) ((x >> (8 * k)) & 255u);
                            if (off > 1 || off < -1) within_bad++;
                            if (exact && off != 0) exact_bad++;
                        }
                    }
        if (exact) {
            for (uint32_t x = 0; x < (1u << 24); x++, full++)
                if (grade_pixel(x, lut.data(), N) != x) full_bad++;
        }
    }
    printf("identity: lattice %ld, beyond one %ld, exact sizes %ld, inexact on the lattice %ld, all colours %ld, inexact %ld\n", lattice, within_bad, exact_sizes, exact_bad, full, full_bad);
    return within_bad || exact_bad || full_bad ? 1 : 0;
}

static bool numbers(char* at, long n, std::vector<long>* out)
{
    while (*at) {
        out->push_back(strtol(at, &at, 10));
        if (*at == ',') at++;
    }
    return (long) out->size() == n;
}

static int grade_frames(int argc, char** argv)
{
    if (argc != 10) return 2;
    const long W = atol(argv[2]), H = atol(argv[3]), stride = atol(argv[4]), n = atol(argv[5]), N = atol(argv[6]);
    if (W < 1 || W > kMaxSide || H < 1 || H > kMaxSide || stride < 3 * W || n < 1 || N < kMinNodes || N > kMaxNodes) return 2;
    std::vector<long> ss;
    if (!numbers(argv[7], n, &ss)) return 2;
    std::vector<uint8_t> in((size_t) (n * H * stride));
    std::vector<uint32_t> lut((size_t) (N * N * N));
    FILE* file = fopen(argv[8], "rb");
    if (!file || fread(in.data(), 1, in.size(), file) != in.size() || fread(lut.data(), 4, lut.size(), file) != lut.size()) return 3;
    fclose(file);
    for (long i = 0; i < n; i++) {
        if (ss[i] < 0 || ss[i] > kMaxStrength) return 2;
        if (ss[i] == 0) continue;
        for (long y = 0; y < H; y++) {
            const size_t at = (size_t) ((i * H + y) * stride);
            grade_row(in.data() + at, (int32_t) W, lut.data(), (uint32_t) N, (uint32_t) ss[i], (uint32_t) (at & 3u));
        }
    }
    file = fopen(argv[9], "wb");
    if (!file || fwrite(in.data(), 1, in.size(), file) != in.size()) return 3;
    fclose(file);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "brute")) return brute((uint32_t) atol(argv[2]));
    if (argc == 2 && !strcmp(argv[1], "forms")) return forms();
    if (argc == 2 && !strcmp(argv[1], "identity")) return identity();
    if (argc >= 2 && !strcmp(argv[1], "grade")) return grade_frames(argc, argv);
    fprintf(stderr, "usage: grade_check brute N | forms | identity | grade W H stride n N s0,s1,... in.raw out.raw\n");
    return 2;
}
