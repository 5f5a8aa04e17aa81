/* kbe_jpeg.cpp -- libkbe_jpeg.so: the frame writers' JPEG encoder (include/kbe_jpeg.h).  HOST code, no GPU; C++ without the STL,
 * exceptions or RTTI, behind a C ABI.
 *
 * Where it sits: the reference hands its finished frames to moviepy -> ffmpeg (`mpeg4`, /root/reference/utils/pipeline.py:130-134).
 * Without an ffmpeg binary this package writes the video itself as Motion-JPEG (pipeline.write_mjpeg_mp4 / _avi), and until
 * round 6 Pillow encoded the frames -- one at a time whatever the thread count (its encoder holds the interpreter lock):
 * 137 ms for the 127 frames of a 512 x 512 video whose three networks and 64 rendered frames take 19 ms.  The frames of a
 * Motion-JPEG stream are independent: this encoder takes a batch of them and spreads it over host threads.
 *
 * What it writes is defined in kbe_mjpeg_block.h, the one definition it shares with the device encoder (kbe_mjpeg.hip): the tables and the
 * header bytes (without restart intervals), the colour conversion, the 1-D DCT, the quantiser, the run-length coder -- the same choices,
 * table for table, as Pillow's default `save(format='JPEG', quality=q)` (tests/test_jpeg_writer.py reads both files' DQT / DHT segments
 * and compares; it decodes this encoder's output with Pillow and holds it against the source, and pins its bytes).
 * This file's own: an MCU's pixels staged as float planes, the DCT's passes taken over eight columns at once (which leaves the block
 * transposed), a 64-bit bit writer that stores four bytes at a time, and the threads.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "kbe_jpeg.h"
#include "kbe_mjpeg_block.h"

using namespace kbe_mjpeg;

/* the hot function is compiled twice, for AVX2 and for the baseline ISA, and picked at load time (the machine that builds the library is
 * not the machine that runs it: no -march=native).  No FMA: with contraction off (the streams' definition) nothing would use it.  The
 * header's helpers are plain `inline`, and one left out of line is compiled for the baseline ISA alone.  As built, every helper with
 * floats in it (luma, chroma_b, chroma_r, average4, fdct8, quantise) is inlined into both clones and the DCT is 8-wide vector code in the
 * AVX2 one; kbe_mjpeg::encode_block<Bits> stays out of line: integer code, for which "avx2" selects no other instruction.  Look at the
 * disassembly again after an edit here. */
#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
#define KBE_HOT __attribute__((target_clones("avx2", "default")))
#else
#define KBE_HOT
#endif

typedef float v8f __attribute__((vector_size(32)));     /* one row of a block: fdct8 on eight of them transforms the eight columns */

/* a call's tables: the shared ones, and what the transposed block the DCT leaves is read through */
struct HostTables {
    Tables t;
    int header_bytes;
    float rq_t[2][64];          /* Tables::rq, transposed */
    uint8_t scan_t[64];         /* position in the zig-zag scan -> index in the transposed block */
};

static void host_tables_build(int w, int h, int quality, HostTables* ht)
{
    ht->header_bytes = host::tables_build(w, h, quality, &ht->t, 0);
    for (int i = 0; i < 64; i++) {
        const int tr = (i & 7) * 8 + (i >> 3);
        ht->rq_t[0][tr] = ht->t.rq[0][i];
        ht->rq_t[1][tr] = ht->t.rq[1][i];
        ht->scan_t[ht->t.scan_of[i]] = (uint8_t) tr;
    }
}

/* the 2-D transform: columns, transpose, columns -- the result is the TRANSPOSED coefficient block (out[v][u]) */
static inline __attribute__((always_inline)) void fdct(float* blk)
{
    v8f d[8], t[8];
    memcpy(d, blk, sizeof(d));
    fdct8(d);
    for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) t[x][y] = d[y][x];
    fdct8(t);
    memcpy(blk, t, sizeof(t));
}

/* the entropy-coded segment: bits gather in a 64-bit word and leave four bytes at a time -- in one store when none of the four is 0xFF
 * (which must be followed by a stuffed zero byte, B.1.1.5), byte by byte otherwise or near the end of the buffer */
struct Bits {
    uint8_t* p; uint8_t* end; uint64_t acc; int n; int overflow;

    void put_byte(unsigned v)
    {
        if (p < end) *p++ = (uint8_t) v; else overflow = 1;
    }
    /* what kbe_mjpeg::encode_block hands its codes and value bits to */
    __attribute__((always_inline)) void bits(unsigned code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const uint32_t v = (uint32_t) (acc >> (n - 32));
            n -= 32;
            if (!(((~v) - 0x01010101u) & v & 0x80808080u) && end - p >= 4) {          /* no byte of v is 0xFF (no byte of ~v is zero) */
                p[0] = (uint8_t) (v >> 24); p[1] = (uint8_t) (v >> 16); p[2] = (uint8_t) (v >> 8); p[3] = (uint8_t) v;
                p += 4;
            } else {
                for (int s = 24; s >= 0; s -= 8) {
                    const unsigned byte = (v >> s) & 0xFFu;
                    put_byte(byte);
                    if (byte == 0xFFu) put_byte(0);
                }
            }
        }
    }
    /* what is left in the word at the end of the scan, the last byte padded with ones (F.1.2.3) */
    void flush()
    {
        if (n & 7) { const int pad = 8 - (n & 7); acc = (acc << pad) | ((1u << pad) - 1u); n += pad; }
        while (n >= 8) {
            const unsigned byte = (unsigned) (acc >> (n - 8)) & 0xFFu;
            put_byte(byte);
            if (byte == 0xFFu) put_byte(0);
            n -= 8;
        }
    }
};

/* one block: the transform, the quantiser, the scan, the shared coder; `pred`: the component's DC value, before and after */
static inline __attribute__((always_inline)) void encode_block(Bits& b, float* blk, const HostTables* ht, int c, int* pred)
{
    int16_t nat[64], zz[64];
    fdct(blk);
    for (int i = 0; i < 64; i++) nat[i] = (int16_t) quantise(blk[i], ht->rq_t[c][i]);         /* (blk and rq_t both hold the transposed block) */
    for (int i = 0; i < 64; i++) zz[i] = nat[ht->scan_t[i]];
    kbe_mjpeg::encode_block(b, zz, ht->t.dc[c], ht->t.ac[c], *pred, nullptr);
    *pred = zz[0];
}

extern "C" size_t kbe_jpeg_bound(int w, int h)
{
    if (w <= 0 || h <= 0) return 0;
    const size_t mcus = (size_t) ((w + 15) / 16) * (size_t) ((h + 15) / 16);
    return 1024 + mcus * 6 * 64 * 4;                            /* headers + 4 bytes per coefficient: see kbe_jpeg.h */
}

KBE_HOT static int encode_one(const uint8_t* rgb, int w, int h, int stride, const HostTables* ht, uint8_t* out, size_t cap, size_t* size)
{
    Bits b = { out, out + cap, 0, 0, 0 };
    for (int i = 0; i < ht->header_bytes; i++) b.put_byte(ht->t.header[i]);
    int pred[3] = { 0, 0, 0 };
    float blocks[6][64];                                                                        /* Y, Y, Y, Y, Cb, Cr */
    for (int my = 0; my < h; my += 16)
        for (int mx = 0; mx < w; mx += 16) {
            /* the MCU's 16 x 16 pixels (edge pixels repeated past the image) as three float planes, colour conversion, chroma averaged 2 x 2 */
            float r[16][16], g[16][16], bl[16][16], yy[16][16], cb[16][16], cr[16][16];
            const int inside = mx + 16 <= w && my + 16 <= h;
            for (int y = 0; y < 16; y++) {
                const uint8_t* row = rgb + (size_t) (my + y < h ? my + y : h - 1) * (size_t) stride;
                if (inside) {
                    const uint8_t* p = row + 3 * (size_t) mx;
                    for (int x = 0; x < 16; x++) { r[y][x] = p[3 * x]; g[y][x] = p[3 * x + 1]; bl[y][x] = p[3 * x + 2]; }
                } else
                    for (int x = 0; x < 16; x++) {
                        const uint8_t* p = row + 3 * (size_t) (mx + x < w ? mx + x : w - 1);
                        r[y][x] = p[0]; g[y][x] = p[1]; bl[y][x] = p[2];
                    }
            }
            for (int y = 0; y < 16; y++)
                for (int x = 0; x < 16; x++) {
                    yy[y][x] = luma(r[y][x], g[y][x], bl[y][x]);
                    cb[y][x] = chroma_b(r[y][x], g[y][x], bl[y][x]);
                    cr[y][x] = chroma_r(r[y][x], g[y][x], bl[y][x]);
                }
            for (int k = 0; k < 4; k++)
                for (int y = 0; y < 8; y++) memcpy(&blocks[k][y * 8], &yy[(k >> 1) * 8 + y][(k & 1) * 8], 8 * sizeof(float));
            for (int y = 0; y < 8; y++)
                for (int x = 0; x < 8; x++) {
                    blocks[4][y * 8 + x] = average4(cb[2 * y][2 * x], cb[2 * y][2 * x + 1], cb[2 * y + 1][2 * x], cb[2 * y + 1][2 * x + 1]);
                    blocks[5][y * 8 + x] = average4(cr[2 * y][2 * x], cr[2 * y][2 * x + 1], cr[2 * y + 1][2 * x], cr[2 * y + 1][2 * x + 1]);
                }
            for (int k = 0; k < 6; k++) encode_block(b, blocks[k], ht, k < 4 ? 0 : 1, &pred[k < 4 ? 0 : k - 3]);
        }
    b.flush();
    b.put_byte(0xFF); b.put_byte(0xD9);                                                         /* EOI */
    if (b.overflow) return KBE_JPEG_E_SPACE;
    *size = (size_t) (b.p - out);
    return KBE_JPEG_OK;
}

extern "C" int kbe_jpeg_encode(const uint8_t* rgb, int w, int h, int stride_bytes, int quality, uint8_t* out, size_t cap, size_t* size)
{
    if (!rgb || !out || !size || w <= 0 || h <= 0 || w > 65535 || h > 65535 || stride_bytes < 3 * w) return KBE_JPEG_E_INVALID;
    HostTables ht;
    host_tables_build(w, h, quality, &ht);
    return encode_one(rgb, w, h, stride_bytes, &ht, out, cap, size);
}

struct Batch {
    const uint8_t* const* rgb; uint8_t* const* outs; size_t* sizes; size_t cap;
    int n, w, h, stride; const HostTables* ht; int next; int status; pthread_mutex_t mu;
};

static void* batch_worker(void* arg)
{
    Batch* b = (Batch*) arg;
    for (;;) {
        pthread_mutex_lock(&b->mu);
        const int i = b->next < b->n ? b->next++ : -1;
        pthread_mutex_unlock(&b->mu);
        if (i < 0) return NULL;
        const int rc = encode_one(b->rgb[i], b->w, b->h, b->stride, b->ht, b->outs[i], b->cap, &b->sizes[i]);
        if (rc != KBE_JPEG_OK) { pthread_mutex_lock(&b->mu); b->status = rc; pthread_mutex_unlock(&b->mu); }
    }
}

extern "C" int kbe_jpeg_encode_batch(const uint8_t* const* rgb, int n, int w, int h, int stride_bytes, int quality, uint8_t* const* outs, size_t cap, size_t* sizes,
                                     int threads)
{
    if (n < 0 || (n > 0 && (!rgb || !outs || !sizes)) || w <= 0 || h <= 0 || w > 65535 || h > 65535 || stride_bytes < 3 * w) return KBE_JPEG_E_INVALID;
    for (int i = 0; i < n; i++) if (!rgb[i] || !outs[i]) return KBE_JPEG_E_INVALID;
    HostTables ht;
    host_tables_build(w, h, quality, &ht);
    Batch b = { rgb, outs, sizes, cap, n, w, h, stride_bytes, &ht, 0, KBE_JPEG_OK, PTHREAD_MUTEX_INITIALIZER };
    if (threads > n) threads = n;
    if (threads > 256) threads = 256;
    pthread_t tid[256];
    int started = 0;
    for (int k = 1; k < threads; k++)                           /* the caller's thread is one of them */
        if (pthread_create(&tid[started], NULL, batch_worker, &b) == 0) started++;
    batch_worker(&b);
    for (int k = 0; k < started; k++) pthread_join(tid[k], NULL);
    pthread_mutex_destroy(&b.mu);
    return b.status;
}
