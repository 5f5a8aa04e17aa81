// mjpeg_check.cpp -- the CPU twin of the device-side Motion-JPEG encoder: csrc/kbe_mjpeg_block.h compiled by g++ and executed serially
// (tests/test_mjpeg_stream.py, tests/test_mjpeg_gpu.py).  Build: g++ -O2 -std=c++17 -ffp-contract=off -I csrc (no -ffast-math, no -march).
//
//   mjpeg_check encode W H quality flags n in.raw out.bin
//       in.raw: n frames [H][W][3] uint8 back to back; out.bin: their streams back to back.  Prints the streams' sizes, the bound of a
//       stream, R, and how often the rare paths of the format were taken.
//   mjpeg_check encode_packed ...: the same through the kernels' two steps (every block's bits packed on their own, then sent on in order).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_mjpeg_block.h"

struct VectorSink {
    std::vector<uint8_t> bytes;
    void put(unsigned v) { bytes.push_back((uint8_t) v); }
};

int main(int argc, char** argv)
{
    const bool packed = argc == 9 && strcmp(argv[1], "encode_packed") == 0;
    if (argc != 9 || (strcmp(argv[1], "encode") != 0 && !packed)) {
        fprintf(stderr, "usage: mjpeg_check encode W H quality flags n in.raw out.bin\n");
        return 2;
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]), quality = atoi(argv[4]), flags = atoi(argv[5]), n = atoi(argv[6]);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || n <= 0) return 2;
    const size_t frame_bytes = (size_t) W * (size_t) H * 3;
    std::vector<uint8_t> in(frame_bytes * (size_t) n);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) { fprintf(stderr, "cannot read %s\n", argv[7]); return 2; }
    fclose(f);

    kbe_mjpeg::Tables t;
    memset(&t, 0, sizeof(t));
    kbe_mjpeg::host::tables_build(W, H, quality, &t);
    {   // the header's length is the constant the kernels count with
        kbe_mjpeg::Tables probe;
        memset(&probe, 0xEE, sizeof(probe));
        kbe_mjpeg::host::tables_build(W, H, quality, &probe);
        if (probe.header[kbe_mjpeg::kHeaderBytes - 1] == 0xEE || probe.header[kbe_mjpeg::kHeaderBytes] != 0xEE) { fprintf(stderr, "header length != kHeaderBytes\n"); return 1; }
    }
    kbe_mjpeg::Stats st;
    memset(&st, 0, sizeof(st));
    VectorSink sink;
    printf("sizes");
    for (int i = 0; i < n; i++) {
        const size_t before = sink.bytes.size();
        kbe_mjpeg::host::encode_frame(in.data() + frame_bytes * (size_t) i, W, H, 3 * W, flags, t, sink, &st, packed);
        const size_t size = sink.bytes.size() - before;
        if (size > kbe_mjpeg::stream_bound(W, H)) { fprintf(stderr, "frame %d: %zu bytes exceed the bound %zu\n", i, size, kbe_mjpeg::stream_bound(W, H)); return 1; }
        printf(" %zu", size);
    }
    printf("\nbound %zu\nR %d\n", kbe_mjpeg::stream_bound(W, H), kbe_mjpeg::kRestartMcus);
    printf("stats stuffed=%ld noeob=%ld dc11=%ld zrl=%ld rstwrap=%ld\n", st.stuffed, st.blocks_without_eob, st.dc_category_11, st.zrl, st.rst_wraps);
    f = fopen(argv[8], "wb");
    if (!f || fwrite(sink.bytes.data(), 1, sink.bytes.size(), f) != sink.bytes.size()) { fprintf(stderr, "cannot write %s\n", argv[8]); return 2; }
    fclose(f);
    return 0;
}
