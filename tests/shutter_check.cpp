// shutter_check.cpp -- csrc/kbe_shutter_block.h compiled by g++ and executed serially: the packed forms the kernel of kbe_shutter_mean_u8
// computes with, held to the plain definition (tests/test_shutter_stream.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   shutter_check brute
//       for every S in 1..32 and every sum in 0..255 S: mean_of(sum, S) is (2 sum + S) / (2 S), lies within 1/2 of sum / S in exact
//       integers (|2 S out - 2 sum| <= S, ties up), and mean_by_magic gives the same; add() and finish() on dwords: every byte value in every
//       one of the 16 lanes of a piece, S times, and dwords whose four bytes are all 255 at S = 32; realign() at every byte offset against
//       the bytes themselves; mean_row at every pair of classes of the output and the source modulo 16, rows of 1..70 bytes, against the
//       plain form byte by byte.
//   shutter_check mean W H stride S n in.raw out.raw
//       in.raw: n * S frames [H][stride] bytes back to back, the sources of output i at i * S ..; out.raw: n frames [H][3 W].  The output
//       rows are taken at the class (y + i) % 16, the rows of source k at the class of their offset in the file: every row another.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_shutter_block.h"

using namespace kbe_shutter;

static uint32_t lcg(uint32_t* state)
{
    *state = *state * 1664525u + 1013904223u;
    return *state >> 24;
}

static int brute()
{
    long plain_bad = 0, magic_bad = 0, packed_bad = 0, realign_bad = 0, row_bad = 0, sums = 0, rows = 0;
    for (uint32_t S = 1; S <= (uint32_t) kMaxSamples; S++) {
        const uint32_t M = magic(S);
        for (uint32_t sum = 0; sum <= 255u * S; sum++, sums++) {
            const uint32_t out = mean_of(sum, S);
            const long off = 2l * S * out - 2l * sum;                      // 2 S (out - sum / S)
            if (out != (2u * sum + S) / (2u * S) || out > 255u || off > (long) S || off <= -(long) S) plain_bad++;
            if (mean_by_magic(sum, S, M) != out) magic_bad++;
        }
        // every lane of a piece on its own, and all lanes full: S dwords added, finish against the plain form
        for (int lane = 0; lane <= 16; lane++)
            for (uint32_t v = 0; v < 256u; v += lane == 16 ? 255u : 1u) {
                uint8_t bytes[16];
                for (int i = 0; i < 16; i++) bytes[i] = lane == 16 || i == lane ? (uint8_t) v : (uint8_t) (255u - v);
                uint32_t w[4], word[4];
                uint8_t got[16];
                memcpy(w, bytes, 16);
                Acc acc;
                clear(acc);
                for (uint32_t s = 0; s < S; s++) add(acc, w);
                finish(acc, S, M, word);
                memcpy(got, word, 16);
                for (int i = 0; i < 16; i++)
                    if (got[i] != mean_of(S * bytes[i], S) || got[i] != bytes[i]) packed_bad++;
            }
    }
    {   // dwords whose four bytes are all 255, 32 of them
        const uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        uint32_t word[4];
        Acc acc;
        clear(acc);
        for (int s = 0; s < 32; s++) add(acc, w);
        finish(acc, 32u, magic(32u), word);
        for (int d = 0; d < 4; d++)
            if (word[d] != 0xFFFFFFFFu || acc.even[d] != 0x1FE01FE0u || acc.odd[d] != 0x1FE01FE0u) packed_bad++;
    }
    for (uint32_t b = 0; b < 4u; b++) {
        uint8_t bytes[20], got[16];
        for (int i = 0; i < 20; i++) bytes[i] = (uint8_t) (17 * i + 3);
        uint32_t x[5], w[4];
        memcpy(x, bytes, 20);
        realign(x, b, w);
        memcpy(got, w, 16);
        if (memcmp(got, bytes + b, 16) != 0) realign_bad++;
    }
    // rows: three samples of noise, every class of the output and of the first source; the other sources a class further on each
    uint32_t state = 7u;
    for (long n = 1; n <= 70; n++)
        for (uint32_t lead = 0; lead < 16u; lead++)
            for (uint32_t cls = 0; cls < 16u; cls++, rows++) {
                const uint32_t S = 1u + (uint32_t) ((n + lead + cls) % 3);
                std::vector<uint8_t> src(3 * n), want(n), got(n + 2, 0xEE);
                for (auto& v : src) v = (uint8_t) lcg(&state);
                const uint8_t* ptr[3] = {src.data(), src.data() + n, src.data() + 2 * n};
                const uint32_t classes[3] = {cls, cls + 1u, cls + 2u};
                for (long j = 0; j < n; j++) {
                    uint32_t sum = 0;
                    for (uint32_t s = 0; s < S; s++) sum += ptr[s][j];
                    want[j] = (uint8_t) mean_of(sum, S);
                }
                mean_row(ptr, classes, S, n, lead, got.data() + 1);
                if (memcmp(got.data() + 1, want.data(), n) != 0 || got[0] != 0xEE || got[n + 1] != 0xEE) row_bad++;
            }
    printf("brute: sums %ld, plain mismatches %ld, multiply-high mismatches %ld, packed mismatches %ld, realign mismatches %ld, rows %ld, row mismatches %ld\n",
           sums, plain_bad, magic_bad, packed_bad, realign_bad, rows, row_bad);
    return plain_bad || magic_bad || packed_bad || realign_bad || row_bad ? 1 : 0;
}

static int mean(int argc, char** argv)
{
    if (argc != 9) return 2;
    const long W = atol(argv[2]), H = atol(argv[3]), stride = atol(argv[4]), S = atol(argv[5]), n = atol(argv[6]);
    if (W < 1 || H < 1 || stride < 3 * W || S < 1 || S > kMaxSamples || n < 1) return 2;
    std::vector<uint8_t> in((size_t) n * S * H * stride), out((size_t) n * H * 3 * W);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
    fclose(f);
    for (long i = 0; i < n; i++)
        for (long y = 0; y < H; y++) {
            const uint8_t* rows[kMaxSamples];
            uint32_t classes[kMaxSamples];
            for (long s = 0; s < S; s++) {
                const size_t at = ((size_t) (i * S + s) * H + y) * stride;
                rows[s] = in.data() + at;
                classes[s] = (uint32_t) (at & 15u);
            }
            mean_row(rows, classes, (uint32_t) S, 3 * W, (uint32_t) ((y + i) % 16), out.data() + ((size_t) i * H + y) * 3 * W);
        }
    f = fopen(argv[8], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "brute")) return brute();
    if (argc >= 2 && !strcmp(argv[1], "mean")) return mean(argc, argv);
    fprintf(stderr, "usage: shutter_check brute | mean W H stride S n in.raw out.raw\n");
    return 2;
}
