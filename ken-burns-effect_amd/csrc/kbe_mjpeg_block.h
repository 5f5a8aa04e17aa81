// kbe_mjpeg_block.h -- the project's ONE definition of its baseline JPEG: the arithmetic and the stream format of both Motion-JPEG encoders.
// Three compilations read it: hipcc into the kernels of kbe_mjpeg.hip (the device encoder), g++ into tests/mjpeg_check.cpp (the device
// encoder's CPU twin, whose encode_frame below runs the same pieces one after the other), and g++ into kbe_jpeg.cpp (libkbe_jpeg.so, the
// host encoder on threads).  The device's stream is, byte for byte, what encode_frame writes (tests/test_mjpeg_gpu.py).
//
// The picture: baseline sequential DCT (ISO/IEC 10918-1), 8 bits, JFIF YCbCr 4:2:0, the Annex K.1 tables under the IJG quality rule, the
// Annex K.3 Huffman tables, edge pixels repeated into partial MCUs.  The host encoder takes from here the constants, the tables, the header
// bytes, the colour conversion, the 1-D DCT, the quantiser and the run-length coder; its own are the order of its DCT passes, its 64-bit bit
// writer and its threads (kbe_jpeg.cpp).  The device encoder adds RESTART INTERVALS: a DRI segment declares intervals of kRestartMcus MCUs;
// every interval starts on a byte boundary with the DC predictors at 0, ends padded with 1-bits and is followed by RSTm, m = 0..7 in turn
// (none after the last).  Intervals are then independent: the unit of work of the kernels.
//
// Every fp32 operation here is one IEEE add, sub or mul (no contraction: -ffp-contract=off on both compilers), every conversion exact.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_MJ_HD __host__ __device__ __forceinline__
#else
#define KBE_MJ_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace kbe_mjpeg {

constexpr int kRestartMcus = 4;         // R: MCUs per restart interval (1024^2, quality 92: +1.7 % bytes against a stream without intervals)
constexpr int kHeaderBytes = 629;       // SOI, APP0, 2 x DQT, SOF0, 4 x DHT, DRI, SOS
constexpr int kFlagBgr = 1;             // KBE_MJPEG_BGR: the frames hold B, G, R

// what the rare paths of a stream were taken by (the host checker prints them; the kernels pass nullptr)
struct Stats { long stuffed, blocks_without_eob, dc_category_11, zrl, rst_wraps; };

struct Tables {
    float rq[2][64];            // 1 / (q * the AAN scale factors * 8), natural order: what a DCT output is multiplied by
    uint32_t dc[2][12];         // Huffman code << 5 | length, by DC category
    uint32_t ac[2][256];        // ... by run << 4 | size
    uint8_t scan_of[64];        // natural index -> position in the zig-zag scan
    uint8_t header[kHeaderBytes + 3];
};

struct Geometry {
    int W, H, stride, bgr;
    int mcus_x, mcus;           // MCUs per row, per frame
    int intervals;              // restart intervals per frame
};

KBE_MJ_HD Geometry geometry(int W, int H, int stride, int flags)
{
    Geometry g;
    g.W = W; g.H = H; g.stride = stride; g.bgr = (flags & kFlagBgr) != 0;
    g.mcus_x = (W + 15) / 16;
    g.mcus = g.mcus_x * ((H + 15) / 16);
    g.intervals = (g.mcus + kRestartMcus - 1) / kRestartMcus;
    return g;
}

// bytes that hold ANY W x H frame's stream.  A block: a DC code of at most 11 bits + 11 value bits, 63 AC codes of at most 16 + 10 bits =
// 1660 bits, 208 bytes; every byte may be 0xFF and then takes a stuffed zero; an interval adds its padded byte (stuffed) and a marker.
KBE_MJ_HD size_t stream_bound(int W, int H)
{
    if (W <= 0 || H <= 0) return 0;
    const Geometry g = geometry(W, H, 0, 0);
    return (size_t) kHeaderBytes + (size_t) g.mcus * 6 * 2 * 208 + (size_t) g.intervals * 4 + 2;
}

// ---------------------------------------------------------------------------------------
// samples: colour conversion (JFIF), 2 x 2 chroma average
// ---------------------------------------------------------------------------------------
KBE_MJ_HD float luma(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b - 128.0f; }
KBE_MJ_HD float chroma_b(float r, float g, float b) { return -0.168735892f * r - 0.331264108f * g + 0.5f * b; }
KBE_MJ_HD float chroma_r(float r, float g, float b) { return 0.5f * r - 0.418687589f * g - 0.081312411f * b; }
// a chroma sample: the 2 x 2 pixels under it, top left, top right, bottom left, bottom right
KBE_MJ_HD float average4(float a, float b, float c, float d) { return 0.25f * (a + b + c + d); }

// component 0..3: the MCU's four luma blocks, 4: Cb, 5: Cr, of one pixel (x, y clamped to the image: edge pixels repeat)
KBE_MJ_HD float sample(const uint8_t* frame, const Geometry& g, int x, int y, int comp)
{
    x = x < g.W ? x : g.W - 1;
    y = y < g.H ? y : g.H - 1;
    const uint8_t* p = frame + (size_t) y * (size_t) g.stride + 3 * (size_t) x;
    const float r = (float) p[g.bgr ? 2 : 0], gr = (float) p[1], b = (float) p[g.bgr ? 0 : 2];
    return comp < 4 ? luma(r, gr, b) : comp == 4 ? chroma_b(r, gr, b) : chroma_r(r, gr, b);
}

// row `r` of block `comp` of the MCU at (mx, my): eight samples
KBE_MJ_HD void block_row(const uint8_t* frame, const Geometry& g, int mx, int my, int comp, int r, float v[8])
{
    if (comp < 4) {
        const int y = my * 16 + (comp >> 1) * 8 + r, x0 = mx * 16 + (comp & 1) * 8;
        for (int j = 0; j < 8; j++) v[j] = sample(frame, g, x0 + j, y, comp);
    } else {
        const int y = my * 16 + 2 * r, x0 = mx * 16;
        for (int j = 0; j < 8; j++)
            v[j] = average4(sample(frame, g, x0 + 2 * j, y, comp), sample(frame, g, x0 + 2 * j + 1, y, comp), sample(frame, g, x0 + 2 * j, y + 1, comp),
                            sample(frame, g, x0 + 2 * j + 1, y + 1, comp));
    }
}

// ---------------------------------------------------------------------------------------
// the Arai-Agui-Nakajima forward DCT of eight values, in place; outputs scaled by the factors folded into Tables::rq.  V: float (the
// kernels, the twin), or a vector of floats that takes as many transforms side by side (the host encoder: the eight columns of a block)
// ---------------------------------------------------------------------------------------
template <class V>
KBE_MJ_HD void fdct8(V d[8])
{
    const V t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const V t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const V t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = t10 + t11; d[4] = t10 - t11;
    const V z1 = (t12 + t13) * 0.707106781f;
    d[2] = t13 + z1; d[6] = t13 - z1;
    const V u10 = t4 + t5, u11 = t5 + t6, u12 = t6 + t7;
    const V z5 = (u10 - u12) * 0.382683433f, z2 = 0.541196100f * u10 + z5, z4 = 1.306562965f * u12 + z5, z3 = u11 * 0.707106781f;
    const V z11 = t7 + z3, z13 = t7 - z3;
    d[5] = z13 + z2; d[3] = z13 - z2; d[1] = z11 + z4; d[7] = z11 - z4;
}

// round to nearest, halves away from zero
KBE_MJ_HD int quantise(float coefficient, float rq)
{
    const float v = coefficient * rq;
    return (int) (v + (v < 0.0f ? -0.5f : 0.5f));
}

// column `c` of a block after the row pass (w[i] = row i's output c): the column pass, quantisation, and the zig-zag scan
KBE_MJ_HD void block_column(float w[8], int c, const float* rq, const uint8_t* scan_of, int16_t* zz)
{
    fdct8(w);
    for (int i = 0; i < 8; i++) zz[scan_of[i * 8 + c]] = (int16_t) quantise(w[i], rq[i * 8 + c]);
}

// ---------------------------------------------------------------------------------------
// entropy coding (F.1.2): bits gather in a word and leave as bytes through `sink.put(byte)`; 0xFF is followed by a stuffed zero (B.1.1.5)
// ---------------------------------------------------------------------------------------
struct BitWriter { uint32_t acc; int n; };

template <class Sink>
KBE_MJ_HD void put_byte_stuffed(Sink& sink, unsigned byte, Stats* st)
{
    sink.put(byte);
    if (byte == 0xFFu) { sink.put(0u); if (st) st->stuffed++; }
}

template <class Sink>
KBE_MJ_HD void put_bits(BitWriter& b, Sink& sink, unsigned code, int len, Stats* st)
{
    b.acc = (b.acc << len) | code;              // (at most 7 bits wait: 7 + 16 fit)
    b.n += len;
    while (b.n >= 8) {
        put_byte_stuffed(sink, (b.acc >> (b.n - 8)) & 0xFFu, st);
        b.n -= 8;
    }
}

// the end of an interval: the last byte padded with ones (F.1.2.3)
template <class Sink>
KBE_MJ_HD void flush_bits(BitWriter& b, Sink& sink, Stats* st)
{
    if (b.n) {
        const int pad = 8 - b.n;
        put_byte_stuffed(sink, ((b.acc << pad) | ((1u << pad) - 1u)) & 0xFFu, st);
    }
    b.acc = 0; b.n = 0;
}

KBE_MJ_HD int bit_length(unsigned a) { return a ? 32 - __builtin_clz(a) : 0; }

// One block from its quantised coefficients in scan order, as Huffman codes and value bits handed to `out.bits(code, length)` (length
// <= 16): the DC difference against `pred`, the AC run lengths with ZRL and EOB.  A block's bits depend on nothing but its coefficients
// and the DC value in front of it: the kernels code the blocks of an interval side by side.
template <class Bits>
KBE_MJ_HD void encode_block(Bits& out, const int16_t* zz, const uint32_t* dc, const uint32_t* ac, int pred, Stats* st)
{
    const int diff = (int) zz[0] - pred;
    {
        const int nb = bit_length((unsigned) (diff < 0 ? -diff : diff));
        out.bits(dc[nb] >> 5, (int) (dc[nb] & 31u));
        if (nb) out.bits((unsigned) (diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), nb);
        if (st && nb == 11) st->dc_category_11++;
    }
    int run = 0;
    for (int i = 1; i < 64; i++) {
        int v = zz[i];
        if (v == 0) { run++; continue; }
        while (run > 15) { out.bits(ac[0xF0] >> 5, (int) (ac[0xF0] & 31u)); run -= 16; if (st) st->zrl++; }
        int nb = bit_length((unsigned) (v < 0 ? -v : v));
        if (nb > 10) { nb = 10; v = v < 0 ? -1023 : 1023; }         // (cannot happen with 8-bit samples and q >= 1)
        const uint32_t e = ac[(run << 4) | nb];
        out.bits(e >> 5, (int) (e & 31u));
        out.bits((unsigned) (v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
        run = 0;
    }
    if (run) out.bits(ac[0] >> 5, (int) (ac[0] & 31u));            // EOB
    else if (st) st->blocks_without_eob++;
}

// the DC value in front of block `comp` of MCU `m` of an interval (zz: [MCUs of the interval][6][64]): the block before it of the same
// component -- the four luma blocks of an MCU follow one another --, 0 at the interval's start
KBE_MJ_HD int dc_predictor(const int16_t* zz, int m, int comp)
{
    if (comp >= 1 && comp <= 3) return zz[(m * 6 + comp - 1) * 64];
    if (m == 0) return 0;
    return zz[((m - 1) * 6 + (comp == 0 ? 3 : comp)) * 64];
}

// bits straight into the stream's bytes
template <class Sink>
struct StreamBits {
    BitWriter b;
    Sink& sink;
    Stats* st;
    KBE_MJ_HD void bits(unsigned code, int len) { put_bits(b, sink, code, len, st); }
};

// behind an interval's last block: the padded byte, then RSTm -- or, behind the frame's last interval, EOI
template <class Sink>
KBE_MJ_HD void end_interval(BitWriter& b, Sink& sink, const Geometry& g, int interval, Stats* st)
{
    flush_bits(b, sink, st);
    sink.put(0xFFu);
    if (interval + 1 < g.intervals) {
        sink.put(0xD0u + (unsigned) (interval & 7));
        if (st && interval >= 8 && (interval & 7) == 0) st->rst_wraps++;
    } else
        sink.put(0xD9u);
}

KBE_MJ_HD int interval_mcus(const Geometry& g, int interval)
{
    const int left = g.mcus - interval * kRestartMcus;
    return left < kRestartMcus ? left : kRestartMcus;
}

// restart interval `interval` of a frame from the coefficients of its MCUs (zz: [MCUs of the interval][6][64])
template <class Sink>
KBE_MJ_HD void encode_interval(Sink& sink, const Geometry& g, int interval, const int16_t* zz, const uint32_t (*dc)[12], const uint32_t (*ac)[256], Stats* st)
{
    StreamBits<Sink> out = { { 0u, 0 }, sink, st };
    const int n = interval_mcus(g, interval);
    for (int m = 0; m < n; m++)
        for (int comp = 0; comp < 6; comp++) {
            const int c = comp < 4 ? 0 : 1;
            encode_block(out, zz + (m * 6 + comp) * 64, dc[c], ac[c], dc_predictor(zz, m, comp), st);
        }
    end_interval(out.b, sink, g, interval, st);
}

// The same interval in two steps, the way the kernels take it: every block's bits packed on their own (PackedBits: most significant bit
// first into 32-bit words; kBlockWords hold any block: 11 + 11 + 63 x 26 = 1660 bits), then the blocks' bits sent on, in order, into the
// stream's bytes (replay_bits).  The bytes are encode_interval's (tests/test_mjpeg_stream.py: the twin runs both).
constexpr int kBlockWords = 52;

struct PackedBits {
    uint32_t* words;
    uint64_t acc;
    int n, count;               // bits waiting in acc, words written
    KBE_MJ_HD void bits(unsigned code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) { words[count++] = (uint32_t) (acc >> (n - 32)); n -= 32; }
    }
    // -> the block's length in bits
    KBE_MJ_HD int finish()
    {
        if (n) words[count] = (uint32_t) (acc << (32 - n));
        return count * 32 + n;
    }
};

template <class Bits>
KBE_MJ_HD void replay_bits(Bits& out, const uint32_t* words, int nbits)
{
    for (int done = 0; done < nbits; done += 16) {
        const int take = nbits - done < 16 ? nbits - done : 16;
        out.bits((words[done >> 5] >> (32 - (done & 31) - take)) & ((1u << take) - 1u), take);
    }
}

// ---------------------------------------------------------------------------------------
// host side: the tables from the quality, the header bytes
// ---------------------------------------------------------------------------------------
namespace host {

static const uint8_t ZIGZAG[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
// Annex K.1, natural (row-major) order
static const uint8_t Q_LUMA[64] = { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 };
static const uint8_t Q_CHROMA[64] = { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 };
// Annex K.3: code counts per length 1..16, then the symbols in code order
static const uint8_t DC_LUMA_BITS[16] = { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 };
static const uint8_t DC_CHROMA_BITS[16] = { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 };
static const uint8_t DC_VALS[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
static const uint8_t AC_LUMA_BITS[16] = { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d };
static const uint8_t AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1,
    0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa };
static const uint8_t AC_CHROMA_BITS[16] = { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 };
static const uint8_t AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09,
    0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38,
    0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa };

inline void huffman_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* table)
{
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < bits[len - 1]; i++, k++) table[vals[k]] = (uint32_t) (code++ << 5) | (uint32_t) len;
        code <<= 1;
    }
}

struct HeaderWriter {
    uint8_t* p;
    void byte(unsigned v) { *p++ = (uint8_t) v; }
    void marker(unsigned m, const uint8_t* body, int len)
    {
        byte(0xFF); byte(m);
        if (len >= 0) { byte((unsigned) (len + 2) >> 8); byte((unsigned) (len + 2) & 0xFF); for (int i = 0; i < len; i++) byte(body[i]); }
    }
};

// quality 1..100 (clamped): the IJG rule (jpeg_quality_scaling) on the Annex K.1 tables; the reciprocals in double, rounded once.
// restart_mcus: what the DRI segment declares -- kRestartMcus for the device encoder's stream (kHeaderBytes of header; the default, so that
// a caller that knows nothing of the host encoder reads as it did), 0 for a stream without intervals and without the segment (the host
// encoder's).  -> the header's length
inline int tables_build(int W, int H, int quality, Tables* t, int restart_mcus = kRestartMcus)
{
    static const double aan[8] = { 1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379 };
    if (quality < 1) quality = 1;
    if (quality > 100) quality = 100;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    uint8_t q[2][64];
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < 64; i++) {
            long v = ((long) (c ? Q_CHROMA[i] : Q_LUMA[i]) * scale + 50) / 100;
            if (v < 1) v = 1;
            if (v > 255) v = 255;                                       // baseline: 8-bit entries
            q[c][i] = (uint8_t) v;
            t->rq[c][i] = (float) (1.0 / ((double) v * aan[i >> 3] * aan[i & 7] * 8.0));
        }
    for (int i = 0; i < 64; i++) t->scan_of[ZIGZAG[i]] = (uint8_t) i;
    for (int c = 0; c < 2; c++) {
        for (int i = 0; i < 12; i++) t->dc[c][i] = 0;
        for (int i = 0; i < 256; i++) t->ac[c][i] = 0;
    }
    huffman_codes(DC_LUMA_BITS, DC_VALS, t->dc[0]);
    huffman_codes(DC_CHROMA_BITS, DC_VALS, t->dc[1]);
    huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS, t->ac[0]);
    huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS, t->ac[1]);

    HeaderWriter hw = { t->header };
    hw.marker(0xD8, nullptr, -1);                                                                                       // SOI
    { static const uint8_t jfif[14] = { 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 }; hw.marker(0xE0, jfif, 14); }
    for (int c = 0; c < 2; c++) {                                                                                       // DQT, zig-zag order
        uint8_t body[65];
        body[0] = (uint8_t) c;
        for (int i = 0; i < 64; i++) body[1 + i] = q[c][ZIGZAG[i]];
        hw.marker(0xDB, body, 65);
    }
    {                                                                                                                   // SOF0: 8 bits, Y 2x2, Cb 1x1, Cr 1x1
        const uint8_t sof[15] = { 8, (uint8_t) (H >> 8), (uint8_t) H, (uint8_t) (W >> 8), (uint8_t) W, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1 };
        hw.marker(0xC0, sof, 15);
    }
    {
        const struct { int id; const uint8_t* bits; const uint8_t* vals; int n; } dht[4] = {
            { 0x00, DC_LUMA_BITS, DC_VALS, 12 }, { 0x10, AC_LUMA_BITS, AC_LUMA_VALS, 162 }, { 0x01, DC_CHROMA_BITS, DC_VALS, 12 }, { 0x11, AC_CHROMA_BITS, AC_CHROMA_VALS, 162 } };
        for (int k = 0; k < 4; k++) {
            uint8_t body[1 + 16 + 162];
            body[0] = (uint8_t) dht[k].id;
            for (int i = 0; i < 16; i++) body[1 + i] = dht[k].bits[i];
            for (int i = 0; i < dht[k].n; i++) body[17 + i] = dht[k].vals[i];
            hw.marker(0xC4, body, 17 + dht[k].n);
        }
    }
    if (restart_mcus) { const uint8_t dri[2] = { (uint8_t) (restart_mcus >> 8), (uint8_t) restart_mcus }; hw.marker(0xDD, dri, 2); }        // DRI
    { static const uint8_t sos[10] = { 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 }; hw.marker(0xDA, sos, 10); }
    return (int) (hw.p - t->header);            // (kHeaderBytes with intervals: tests/mjpeg_check.cpp asserts it)
}

// The definition of a frame's stream: the pieces above, one after the other.
// (`packed`: the intervals in the kernels' two steps -- the same bytes)
template <class Sink>
inline void encode_frame(const uint8_t* frame, int W, int H, int stride, int flags, const Tables& t, Sink& sink, Stats* st, bool packed = false)
{
    const Geometry g = geometry(W, H, stride, flags);
    for (int i = 0; i < kHeaderBytes; i++) sink.put(t.header[i]);
    int16_t zz[kRestartMcus * 6 * 64];
    for (int interval = 0; interval < g.intervals; interval++) {
        for (int m = 0; m < kRestartMcus && interval * kRestartMcus + m < g.mcus; m++) {
            const int mcu = interval * kRestartMcus + m, mx = mcu % g.mcus_x, my = mcu / g.mcus_x;
            for (int comp = 0; comp < 6; comp++) {
                float rows[8][8], w[8];
                for (int r = 0; r < 8; r++) { block_row(frame, g, mx, my, comp, r, rows[r]); fdct8(rows[r]); }
                for (int c = 0; c < 8; c++) {
                    for (int i = 0; i < 8; i++) w[i] = rows[i][c];
                    block_column(w, c, t.rq[comp < 4 ? 0 : 1], t.scan_of, zz + (m * 6 + comp) * 64);
                }
            }
        }
        if (!packed) {
            encode_interval(sink, g, interval, zz, t.dc, t.ac, st);
            continue;
        }
        uint32_t words[kRestartMcus * 6][kBlockWords];
        int nbits[kRestartMcus * 6];
        const int blocks = interval_mcus(g, interval) * 6;
        for (int blk = 0; blk < blocks; blk++) {
            PackedBits p = { words[blk], 0, 0, 0 };
            encode_block(p, zz + blk * 64, t.dc[blk % 6 < 4 ? 0 : 1], t.ac[blk % 6 < 4 ? 0 : 1], dc_predictor(zz, blk / 6, blk % 6), st);
            nbits[blk] = p.finish();
        }
        StreamBits<Sink> out = { { 0u, 0 }, sink, st };
        for (int blk = 0; blk < blocks; blk++) replay_bits(out, words[blk], nbits[blk]);
        end_interval(out.b, sink, g, interval, st);
    }
}

}  // namespace host

}  // namespace kbe_mjpeg
