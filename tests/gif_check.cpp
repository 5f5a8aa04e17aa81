// gif_check.cpp -- the CPU twin of the device-side GIF encoder: csrc/kbe_gif_block.h compiled by g++ and executed serially
// (tests/test_gif_stream.py, tests/test_gif_gpu.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   gif_check encode W H flags dither delay_cs n in.raw lut.bin out.bin
//       in.raw: n frames [H][W][3] uint8 back to back; lut.bin: the 32768 bytes of the cell -> index table; out.bin: the frames' units back
//       to back.  Prints the units' sizes, the bound of a unit, the segment size, and how many codes, segments and padding Clears there were.
//   gif_check encode_pieces ...: the same through the kernels' steps (open-addressing dictionary, the byte count from the number of codes, every
//       code placed on its own at its closed-form position, the sub-blocks read back byte by byte).
//   gif_check bound W H
//   gif_check segment
//   gif_check widths K...: code_width(k) and bits_before(k) for every K
//   gif_check sizes W H flags dither n in.raw lut.bin S...
//       the LZW bytes (sub-blocks and all) of the n frames cut into segments of S pixels, for every S (<= 3838), and coded as ONE segment
//       per frame with the usual Clear when the 4096 entries are full: the measurement next to kSegmentPixels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_gif_block.h"

using namespace kbe_gif;

static bool read_file(const char* path, std::vector<uint8_t>& into)
{
    FILE* f = fopen(path, "rb");
    if (!f || fread(into.data(), 1, into.size(), f) != into.size()) { fprintf(stderr, "cannot read %s\n", path); if (f) fclose(f); return false; }
    fclose(f);
    return true;
}

// the data bytes of idx[0 .. n) as ONE LZW stream: a Clear and a fresh table whenever the decoder's table is about to fill
static uint64_t whole_frame_bytes(const uint8_t* idx, uint64_t n, host::DirectTable* dict)
{
    dict->fresh();
    uint64_t bits = 9;                          // the opening Clear
    uint32_t prefix = idx[0], next = kFirstFree, entries = kFirstFree, codes = 0;
    int width = 9;
    auto emitted = [&]() {
        bits += (uint64_t) width;
        if (codes++) entries++;
        if (entries == (1u << width) && width < 12) width++;
    };
    for (uint64_t i = 1; i < n; i++) {
        const uint32_t c = idx[i];
        uint32_t slot;
        const int found = dict->find(prefix, c, &slot);
        if (found >= 0) { prefix = (uint32_t) found; continue; }
        emitted();
        if (next < 4095u) dict->add(prefix, c, next++, slot);
        else { bits += (uint64_t) width; dict->fresh(); next = entries = kFirstFree; codes = 0; width = 9; }
        prefix = c;
    }
    emitted();
    bits += (uint64_t) width;                   // EOI
    const uint64_t bytes = (bits + 7) / 8;
    return bytes + (bytes + 254) / 255;
}

static int sizes_command(int argc, char** argv)
{
    const int W = atoi(argv[2]), H = atoi(argv[3]), flags = atoi(argv[4]), dither = atoi(argv[5]), n = atoi(argv[6]);
    if (unit_bound(W, H) == 0 || n <= 0) return 2;
    const size_t frame_bytes = (size_t) W * (size_t) H * 3, pixels = (size_t) W * (size_t) H;
    std::vector<uint8_t> in(frame_bytes * (size_t) n), lut(kCells), idx(pixels * (size_t) n);
    if (!read_file(argv[7], in) || !read_file(argv[8], lut)) return 2;
    const Geometry g = geometry(W, H, 3 * W, flags, dither);
    for (int f = 0; f < n; f++)
        for (size_t p = 0; p < pixels; p++) idx[(size_t) f * pixels + p] = lut[pixel_cell(in.data() + frame_bytes * (size_t) f, g, p, true)];
    host::DirectTable dict;
    uint64_t whole = 0;
    for (int f = 0; f < n; f++) whole += whole_frame_bytes(idx.data() + (size_t) f * pixels, pixels, &dict);
    printf("whole %llu\n", (unsigned long long) whole);
    for (int a = 9; a < argc; a++) {
        const uint32_t S = (uint32_t) atoi(argv[a]);
        if (S < 1 || S > 3838) return 2;
        uint64_t total = 0;
        for (int f = 0; f < n; f++)
            for (size_t from = 0; from < pixels; from += S) {
                const uint32_t len = pixels - from < S ? (uint32_t) (pixels - from) : S;
                dict.fresh();
                CountCodes count;
                total += segment_bytes(match_loop(idx.data() + (size_t) f * pixels + from, len, dict, count), from == 0, from + len == pixels);
            }
        printf("segment %u bytes %llu ratio %.4f\n", S, (unsigned long long) total, (double) total / (double) whole);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "segment") == 0) { printf("segment %d\n", kSegmentPixels); return 0; }
    if (argc == 4 && strcmp(argv[1], "bound") == 0) { printf("bound %zu\n", unit_bound(atoi(argv[2]), atoi(argv[3]))); return 0; }
    if (argc >= 3 && strcmp(argv[1], "widths") == 0) {
        for (int a = 2; a < argc; a++) { const uint32_t k = (uint32_t) strtoul(argv[a], nullptr, 10); printf("width %u %d %u\n", k, code_width(k), bits_before(k)); }
        return 0;
    }
    if (argc >= 10 && strcmp(argv[1], "sizes") == 0) return sizes_command(argc, argv);
    const bool pieces = argc == 11 && strcmp(argv[1], "encode_pieces") == 0;
    if (argc != 11 || (strcmp(argv[1], "encode") != 0 && !pieces)) {
        fprintf(stderr, "usage: gif_check encode|encode_pieces W H flags dither delay_cs n in.raw lut.bin out.bin | bound W H | segment | widths K... | sizes ...\n");
        return 2;
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]), flags = atoi(argv[4]), dither = atoi(argv[5]), delay = atoi(argv[6]), n = atoi(argv[7]);
    const size_t bound = unit_bound(W, H);
    if (bound == 0 || n <= 0 || dither < 0 || dither > kMaxDither || delay < 0 || delay > 65535) return 2;
    const size_t frame_bytes = (size_t) W * (size_t) H * 3;
    std::vector<uint8_t> in(frame_bytes * (size_t) n), lut(kCells), unit(bound + host::kSegmentRoom + 64), all;
    if (!read_file(argv[8], in) || !read_file(argv[9], lut)) return 2;

    host::Stats st;
    memset(&st, 0, sizeof(st));
    printf("sizes");
    for (int i = 0; i < n; i++) {
        const size_t size = host::encode_frame(in.data() + frame_bytes * (size_t) i, W, H, 3 * W, flags, dither, delay, lut.data(), unit.data(), &st, pieces);
        if (size > bound) { fprintf(stderr, "frame %d: %zu bytes exceed the bound %zu\n", i, size, bound); return 1; }
        all.insert(all.end(), unit.begin(), unit.begin() + size);
        printf(" %zu", size);
    }
    printf("\nbound %zu\nsegment %d\n", bound, kSegmentPixels);
    printf("stats codes=%ld segments=%ld pad_clears=%ld\n", st.codes, st.segments, st.pad_clears);
    FILE* f = fopen(argv[10], "wb");
    if (!f || fwrite(all.data(), 1, all.size(), f) != all.size()) { fprintf(stderr, "cannot write %s\n", argv[10]); return 2; }
    fclose(f);
    return 0;
}
