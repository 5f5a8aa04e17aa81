// png_check.cpp -- the CPU twin of the device-side PNG encoder: csrc/kbe_png_block.h compiled by g++ and executed serially
// (tests/test_png_stream.py, tests/test_png_gpu.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   png_check encode W H flags n in.raw out.bin
//       in.raw: n frames [H][W][3] uint8 back to back; out.bin: their files back to back.  Prints the files' sizes, the bound of a file,
//       the segment size, and how many segments left coded and stored and in how many the length limit cut a code.
//   png_check encode_pieces ...: the same through the kernels' steps (a segment in pieces of 64 bytes, every piece's bits packed at their place).
//   png_check lengths LIMIT COUNT...
//       the code construction on a histogram (COUNT per symbol, at most 286): prints the lengths, whether the limit cut the tree, and
//       the Kraft sum as a fraction of 2^LIMIT.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_png_block.h"

using namespace kbe_png;

static int lengths_command(int argc, char** argv)
{
    const int limit = atoi(argv[2]), nsym = argc - 3;
    if (limit < 1 || limit > kLitLimit || nsym < 1 || nsym > kLitSyms) return 2;
    static Work w;
    for (int i = 0; i < nsym; i++) w.hist[i] = (uint32_t) strtoul(argv[3 + i], nullptr, 10);
    const int used = order_symbols(w.hist, nsym, w.order);
    const int limited = lengths_from_order(w.hist, w.order, used, nsym, limit, w.lit_len, w.weight, w.up, w.count);
    unsigned long kraft = 0;
    printf("lengths");
    for (int i = 0; i < nsym; i++) {
        printf(" %d", w.lit_len[i]);
        if (w.lit_len[i]) kraft += 1ul << (limit - w.lit_len[i]);
    }
    printf("\nlimited %d\nkraft %lu / %lu\n", limited, kraft, 1ul << limit);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 4 && strcmp(argv[1], "lengths") == 0) return lengths_command(argc, argv);
    const bool pieces = argc == 8 && strcmp(argv[1], "encode_pieces") == 0;
    if (argc != 8 || (strcmp(argv[1], "encode") != 0 && !pieces)) {
        fprintf(stderr, "usage: png_check encode W H flags n in.raw out.bin | png_check lengths LIMIT COUNT...\n");
        return 2;
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]), flags = atoi(argv[4]), n = atoi(argv[5]);
    const size_t bound = file_bound(W, H);
    if (bound == 0 || n <= 0) return 2;
    const size_t frame_bytes = (size_t) W * (size_t) H * 3;
    std::vector<uint8_t> in(frame_bytes * (size_t) n), file(bound), all;
    FILE* f = fopen(argv[6], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) { fprintf(stderr, "cannot read %s\n", argv[6]); return 2; }
    fclose(f);

    host::Tables t;
    host::tables_build(W, H, &t);
    host::Stats st;
    memset(&st, 0, sizeof(st));
    printf("sizes");
    for (int i = 0; i < n; i++) {
        const size_t size = host::encode_frame(in.data() + frame_bytes * (size_t) i, W, H, 3 * W, flags, t, file.data(), &st, pieces ? kSegmentBytes / 256 : 0);
        if (size > bound) { fprintf(stderr, "frame %d: %zu bytes exceed the bound %zu\n", i, size, bound); return 1; }
        all.insert(all.end(), file.begin(), file.begin() + size);
        printf(" %zu", size);
    }
    printf("\nbound %zu\nsegment %d\n", bound, kSegmentBytes);
    printf("stats coded=%ld stored=%ld limited_lit=%ld limited_cl=%ld\n", st.coded, st.stored, st.limited_lit, st.limited_cl);
    f = fopen(argv[7], "wb");
    if (!f || fwrite(all.data(), 1, all.size(), f) != all.size()) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
    fclose(f);
    return 0;
}
