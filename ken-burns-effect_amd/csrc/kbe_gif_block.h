// kbe_gif_block.h -- the project's ONE definition of the animated GIF of the device-side encoder (kbe_gif_encode, include/kbe_gif.h).
// Two compilations read it: hipcc into the kernels of kbe_gif.hip, and g++ into tests/gif_check.cpp (the CPU twin, whose encode_frame
// below runs the same pieces one after the other).  The device's unit is, byte for byte, what encode_frame writes (tests/test_gif_gpu.py).
//
// The file (assembled on the host, ken-burns-effect_amd/gif.py): GIF89a, the logical screen descriptor, ONE global colour table of 256
// entries, the NETSCAPE2.0 loop extension, the frames' UNITS back to back, 3B.  A unit is what the device writes, one per frame: a graphic
// control extension (no transparency, no disposal, the delay in centiseconds), an image descriptor (the full frame, no local table, no
// interlace), the minimum code size 08, the LZW data in sub-blocks, 00.  No field of a unit depends on its place in the file.
//
// Pixel -> index, all integers: the channels swapped under kFlagBgr; an ordered dither (bayer8 at x & 7, y & 7, scaled by the amplitude,
// added per channel and clamped: dithered); the RGB555 cell r5 << 10 | g5 << 5 | b5; index = lut[cell] (32 768 bytes in device memory).
//
// LZW in SEGMENTS of kSegmentPixels indices in raster order (the last one short), the unit of work of the kernels: independent, byte-aligned
// and self-framed.  Every segment is coded with a fresh dictionary -- codes 0..255, Clear 256, EOI 257, the first free code 258, 9 bits
// growing to 12 by GIF's rule; kSegmentPixels <= 3838, so the 4096 entries never fill and the corner where decoders differ cannot occur.
// The frame's first segment starts with a Clear.  A segment that is not the last ends with one Clear at the current width and then
// k = (-bits) mod 8 more Clears of 9 bits each (9 k = k mod 8: at most 7 of them restore the byte boundary); the last one ends with EOI
// and zero bits up to the byte.  A segment's bytes go into data sub-blocks of ITS OWN (255 bytes each, the last one short): its byte
// count includes its framing, the counts add up, and the scan of kbe_units_scan.h applies as it is.
//
// The k-th code's width depends on k alone (the table grows by one entry per code): code_width, bits_before and segment_bytes are closed
// forms, so the counting pass needs only a segment's NUMBER of codes and the storing pass packs all codes side by side.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_GIF_HD __host__ __device__ __forceinline__
#else
#define KBE_GIF_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

namespace kbe_gif {

// 1..3838.  512^2 photo-like frames (8 of them, one palette for all; tests/gif_check.cpp: sizes), the LZW bytes against the same indices coded
// as ONE segment per frame (a Clear whenever the 4096 entries are full): 1.099 (512: 1.581, 1024: 1.376, 2048: 1.195, 3072: 1.133; with the
// ordered dither at 8: 1.101, and 1.540 / 1.372 / 1.196 / 1.134).  The largest segment that can never fill the table is also the cheapest
// in bytes, and a 1024^2 frame still has 274 of them.
constexpr int kSegmentPixels = 3838;
static_assert(kSegmentPixels >= 1 && kSegmentPixels <= 3838, "a segment adds at most 3837 entries to the 258: the table never fills");
constexpr int kFlagBgr = 1;             // KBE_GIF_BGR: the frames hold B, G, R
constexpr int kMaxDither = 64;          // the dither's amplitude: 0 (none) .. 64
constexpr int kCells = 32768;           // RGB555
constexpr int kClear = 256, kEoi = 257, kFirstFree = 258;
constexpr int kLeadBytes = 19;          // graphic control extension 8, image descriptor 10, minimum code size 1: in front of a frame's first segment
constexpr int kTailBytes = 1;           // the block terminator behind its last one
constexpr int kHashSlots = 8192;        // the kernels' dictionary (Dictionary below): at most 3837 of them are ever used

struct Geometry {
    int W, H, stride, bgr, dither;
    uint64_t pixels;
    uint32_t segments;
};

KBE_GIF_HD Geometry geometry(int W, int H, int stride, int flags, int dither)
{
    Geometry g;
    g.W = W; g.H = H; g.stride = stride; g.bgr = (flags & kFlagBgr) != 0; g.dither = dither;
    g.pixels = (uint64_t) W * (uint64_t) H;
    g.segments = (uint32_t) ((g.pixels + kSegmentPixels - 1) / kSegmentPixels);
    return g;
}

KBE_GIF_HD uint32_t segment_length(const Geometry& g, uint32_t segment)
{
    const uint64_t left = g.pixels - (uint64_t) segment * kSegmentPixels;
    return left < (uint64_t) kSegmentPixels ? (uint32_t) left : (uint32_t) kSegmentPixels;
}

// ---------------------------------------------------------------------------------------
// pixel -> index
// ---------------------------------------------------------------------------------------
// the 8 x 8 Bayer matrix, 0..63: the bits of (x ^ y, y) interleaved and reversed
KBE_GIF_HD unsigned bayer8(unsigned x, unsigned y)
{
    const unsigned q = x ^ y;
    unsigned m = 0;
    for (int i = 0; i < 3; i++) m |= ((((y >> i) & 1u) << 1) | ((q >> i) & 1u)) << (2 * (2 - i));
    return m;
}

// a channel's value under the dither: + (bayer * amplitude >> 6) - (amplitude >> 1), clamped to 0..255
KBE_GIF_HD unsigned dithered(unsigned v, unsigned bayer, int amplitude)
{
    const int t = (int) v + (int) ((bayer * (unsigned) amplitude) >> 6) - (amplitude >> 1);
    return (unsigned) (t < 0 ? 0 : t > 255 ? 255 : t);
}

KBE_GIF_HD unsigned cell_of(unsigned r, unsigned g, unsigned b)
{
    return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3);
}

// the RGB555 cell of pixel `at` (< g.pixels, raster order) of a frame
KBE_GIF_HD unsigned pixel_cell(const uint8_t* frame, const Geometry& g, uint64_t at, bool dither)
{
    const uint32_t y = (uint32_t) (at / (uint32_t) g.W), x = (uint32_t) (at - (uint64_t) y * (uint32_t) g.W);
    const uint8_t* p = frame + (size_t) y * (size_t) g.stride + 3 * (size_t) x;
    unsigned r = p[g.bgr ? 2 : 0], gr = p[1], b = p[g.bgr ? 0 : 2];
    if (dither && g.dither) {
        const unsigned m = bayer8(x & 7u, y & 7u);
        r = dithered(r, m, g.dither); gr = dithered(gr, m, g.dither); b = dithered(b, m, g.dither);
    }
    return cell_of(r, gr, b);
}

// a cell's centre colour per channel: (v5 << 3) | (v5 >> 2)
KBE_GIF_HD unsigned cell_centre(unsigned v5) { return (v5 << 3) | (v5 >> 2); }

// lut[cell]: the palette entry (3 bytes each, n >= 1 of them) nearest to the cell's centre, squared Euclidean distance, ties to the lowest index
KBE_GIF_HD unsigned nearest_entry(const uint8_t* palette, int n, unsigned cell)
{
    const int r = (int) cell_centre((cell >> 10) & 31u), g = (int) cell_centre((cell >> 5) & 31u), b = (int) cell_centre(cell & 31u);
    unsigned best = 0;
    int best_d = 0x7FFFFFFF;
    for (int i = 0; i < n; i++) {
        const int dr = r - palette[3 * i], dg = g - palette[3 * i + 1], db = b - palette[3 * i + 2];
        const int d = dr * dr + dg * dg + db * db;
        if (d < best_d) { best_d = d; best = (unsigned) i; }
    }
    return best;
}

// ---------------------------------------------------------------------------------------
// the code stream's closed forms.  After k data codes the decoder's table holds 258 + max(k - 1, 0) entries (the first code of a fresh
// dictionary adds none), and the NEXT code -- data, Clear or EOI -- has the width of that table: 9 bits below 512 entries, 10 below
// 1024, 11 below 2048, else 12.
// ---------------------------------------------------------------------------------------
KBE_GIF_HD int code_width(uint32_t k)
{
    const uint32_t entries = (uint32_t) kFirstFree + (k ? k - 1u : 0u);
    return 9 + (entries >= 512u) + (entries >= 1024u) + (entries >= 2048u);
}

// the bits of data codes 0 .. k-1: codes 0..254 take 9 bits, 255..766 take 10, 767..1790 take 11, the rest 12
KBE_GIF_HD uint32_t bits_before(uint32_t k)
{
    return 9u * k + (k > 255u ? k - 255u : 0u) + (k > 767u ? k - 767u : 0u) + (k > 1791u ? k - 1791u : 0u);
}

// what a segment of m data codes takes, in bits up to and with its closing code (Clear or EOI), and how many 9-bit Clears pad it
KBE_GIF_HD uint32_t segment_bits(uint32_t m, bool first, bool last, uint32_t* pad_clears)
{
    const uint32_t bits = (first ? 9u : 0u) + bits_before(m) + (uint32_t) code_width(m);
    *pad_clears = last ? 0u : (0u - bits) & 7u;
    return bits;
}

// ... in bytes without the sub-blocks' length bytes, and with them
KBE_GIF_HD uint32_t segment_data_bytes(uint32_t m, bool first, bool last)
{
    uint32_t pad;
    const uint32_t bits = segment_bits(m, first, last, &pad);
    return (bits + 9u * pad + 7u) / 8u;
}

KBE_GIF_HD uint32_t framed_bytes(uint32_t data_bytes) { return data_bytes + (data_bytes + 254u) / 255u; }

KBE_GIF_HD uint32_t segment_bytes(uint32_t m, bool first, bool last) { return framed_bytes(segment_data_bytes(m, first, last)); }

// byte f (< framed_bytes(n)) of n data bytes in sub-blocks of 255: a length byte at every multiple of 256, the data between them
template <class Data>
KBE_GIF_HD unsigned framed_byte(const Data& data, uint32_t n, uint32_t f)
{
    const uint32_t block = f >> 8, in = f & 255u;
    if (in == 0) { const uint32_t left = n - 255u * block; return left < 255u ? left : 255u; }
    return data(255u * block + in - 1u);
}

// bytes that hold ANY W x H frame's unit: every data code covers one pixel.  0: a size the encoder refuses (the unit would not stay below 2^31 bytes)
KBE_GIF_HD size_t unit_bound(int W, int H)
{
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return 0;
    const Geometry g = geometry(W, H, 0, 0, 0);
    const uint32_t last_n = segment_length(g, g.segments - 1);
    uint64_t bound = (uint64_t) kLeadBytes + kTailBytes;
    if (g.segments == 1) bound += segment_bytes(last_n, true, true);
    else bound += (uint64_t) segment_bytes(kSegmentPixels, true, false) + (uint64_t) (g.segments - 2) * segment_bytes(kSegmentPixels, false, false) + segment_bytes(last_n, false, true);
    return bound < (1ull << 31) ? (size_t) bound : 0;
}

// a unit's first kLeadBytes
KBE_GIF_HD void lead_bytes(int W, int H, int delay_cs, uint8_t* out)
{
    const uint8_t lead[kLeadBytes] = { 0x21, 0xF9, 0x04, 0x00, (uint8_t) delay_cs, (uint8_t) (delay_cs >> 8), 0x00, 0x00,
                                       0x2C, 0, 0, 0, 0, (uint8_t) W, (uint8_t) (W >> 8), (uint8_t) H, (uint8_t) (H >> 8), 0x00, 0x08 };
    for (int i = 0; i < kLeadBytes; i++) out[i] = lead[i];
}

// ---------------------------------------------------------------------------------------
// LZW.  The dictionary's semantics are the format's: (prefix code, byte) -> code, entries in the order they are added.  Which map holds
// them does not show in the stream: the kernels take Dictionary (open addressing in LDS), the twin's definition a direct table.
// ---------------------------------------------------------------------------------------
// kHashSlots words, one entry each: prefix << 20 | byte << 12 | code; kEmpty: none (code 4095 is never given out)
struct Dictionary {
    uint32_t* slots;
    static constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    KBE_GIF_HD static uint32_t home(uint32_t key) { return (key * 2654435761u) >> 19; }
    // the code of (prefix, byte), or -1 and *free_slot: where add() puts it
    KBE_GIF_HD int find(uint32_t prefix, uint32_t byte, uint32_t* free_slot) const
    {
        const uint32_t key = (prefix << 8) | byte;
        uint32_t at = home(key);
        for (int probe = 0; probe < kHashSlots; probe++, at = (at + 1u) & (uint32_t) (kHashSlots - 1)) {
            const uint32_t s = slots[at];
            if (s == kEmpty) break;
            if ((s >> 12) == key) return (int) (s & 0xFFFu);
        }
        *free_slot = at;
        return -1;
    }
    KBE_GIF_HD void add(uint32_t prefix, uint32_t byte, uint32_t code, uint32_t free_slot) { slots[free_slot] = (((prefix << 8) | byte) << 12) | code; }
};
static_assert((kHashSlots & (kHashSlots - 1)) == 0 && kHashSlots == 1 << 13, "home() keeps 13 bits");

// the data codes of indices idx[0 .. n), n >= 1, with a fresh (empty) dictionary: out.code(k, value) for k = 0, 1 ... -> their number
template <class Dict, class Out>
KBE_GIF_HD uint32_t match_loop(const uint8_t* idx, uint32_t n, Dict& dict, Out& out)
{
    uint32_t prefix = idx[0], next = (uint32_t) kFirstFree, k = 0;
    for (uint32_t i = 1; i < n; i++) {
        const uint32_t c = idx[i];
        uint32_t slot = 0;
        const int found = dict.find(prefix, c, &slot);
        if (found >= 0) { prefix = (uint32_t) found; continue; }
        out.code(k++, prefix);
        dict.add(prefix, c, next++, slot);
        prefix = c;
    }
    out.code(k++, prefix);
    return k;
}

struct CountCodes {
    KBE_GIF_HD void code(uint32_t, uint32_t) {}
};

struct KeepCodes {
    uint16_t* codes;
    KBE_GIF_HD void code(uint32_t k, uint32_t value) { codes[k] = (uint16_t) value; }
};

// bits into zeroed 32-bit words from bit `at` on, least significant bit first (GIF packs its codes that way): a value leaves through
// words.merge(index, value) -- an OR, atomic in LDS, because a word holds the bits of several lanes' codes
template <class Words>
KBE_GIF_HD void put_bits(Words& words, uint32_t at, uint32_t value, int width)
{
    const uint64_t v = (uint64_t) value << (at & 31u);
    words.merge(at >> 5, (uint32_t) v);
    if ((at & 31u) + (uint32_t) width > 32u) words.merge((at >> 5) + 1u, (uint32_t) (v >> 32));
}

// piece j of a segment's bits, j = 0 .. m + 1 + pad (any order, any lane): the frame's opening Clear (j = 0, first segments only), data
// code j - 1, the closing code, the padding Clears
template <class Words>
KBE_GIF_HD void put_piece(Words& words, const uint16_t* codes, uint32_t m, bool first, bool last, uint32_t j)
{
    const uint32_t lead = first ? 9u : 0u;
    if (j == 0) { if (first) put_bits(words, 0u, (uint32_t) kClear, 9); return; }
    const uint32_t k = j - 1u;
    if (k < m) put_bits(words, lead + bits_before(k), codes[k], code_width(k));
    else if (k == m) put_bits(words, lead + bits_before(m), last ? (uint32_t) kEoi : (uint32_t) kClear, code_width(m));
    else put_bits(words, lead + bits_before(m) + (uint32_t) code_width(m) + 9u * (k - m - 1u), (uint32_t) kClear, 9);
}

// ---------------------------------------------------------------------------------------
// host side: the definition of a frame's unit
// ---------------------------------------------------------------------------------------
namespace host {

// (prefix, byte) -> code in a table of its own kind: 4096 x 256 entries, the touched ones remembered so that a fresh dictionary is cheap
struct DirectTable {
    uint16_t* table;            // 0: none (code 0 is never an entry's)
    uint32_t* touched;
    uint32_t n_touched;
    DirectTable() : table(new uint16_t[4096 * 256]()), touched(new uint32_t[4096]), n_touched(0) {}
    ~DirectTable() { delete[] table; delete[] touched; }
    void fresh() { while (n_touched) table[touched[--n_touched]] = 0; }
    int find(uint32_t prefix, uint32_t byte, uint32_t* free_slot) const
    {
        *free_slot = (prefix << 8) | byte;
        return table[*free_slot] ? (int) table[*free_slot] : -1;
    }
    void add(uint32_t, uint32_t, uint32_t code, uint32_t free_slot) { table[free_slot] = (uint16_t) code; touched[n_touched++] = free_slot; }
};

// bits into bytes, least significant bit first
struct ByteBits {
    uint8_t* bytes;
    uint64_t acc;
    int n;
    uint32_t count;
    void bits(uint32_t v, int len)
    {
        acc |= (uint64_t) v << n;
        n += len;
        while (n >= 8) { bytes[count++] = (uint8_t) acc; acc >>= 8; n -= 8; }
    }
    void flush() { if (n) { bytes[count++] = (uint8_t) acc; acc = 0; n = 0; } }
};

struct PlainWords {
    uint32_t* w;
    void merge(uint32_t index, uint32_t value) { w[index] |= value; }
};

struct Stats { long codes, segments, pad_clears; };

constexpr uint32_t kSegmentRoom = (9 + 12 * (kSegmentPixels + 1) + 63 + 7) / 8;         // a segment's data bytes at most

// one segment's indices idx[0 .. n) into out (room: framed_bytes(kSegmentRoom)) -> its bytes, sub-blocks and all.  Written the plain
// way: the codes one after the other at the width the decoder's table has, then the sub-blocks
inline uint32_t encode_segment(const uint8_t* idx, uint32_t n, bool first, bool last, uint8_t* out, DirectTable* dict, Stats* st)
{
    static uint16_t codes[kSegmentPixels];
    static uint8_t data[kSegmentRoom + 8];
    dict->fresh();
    KeepCodes keep = { codes };
    const uint32_t m = match_loop(idx, n, *dict, keep);
    ByteBits bits = { data, 0, 0, 0 };
    if (first) bits.bits((uint32_t) kClear, 9);
    uint32_t entries = (uint32_t) kFirstFree;
    int width = 9;
    for (uint32_t k = 0; k < m; k++) {
        bits.bits(codes[k], width);
        if (k) entries++;                                           // (what the decoder adds on reading code k)
        if (entries == (1u << width) && width < 12) width++;
    }
    uint32_t pad = 0;
    if (last) { bits.bits((uint32_t) kEoi, width); bits.flush(); }
    else {
        bits.bits((uint32_t) kClear, width);
        while (bits.n) { bits.bits((uint32_t) kClear, 9); pad++; }
    }
    if (st) { st->codes += m; st->segments++; st->pad_clears += pad; }
    uint32_t at = 0;
    for (uint32_t from = 0; from < bits.count; from += 255u) {
        const uint32_t len = bits.count - from < 255u ? bits.count - from : 255u;
        out[at++] = (uint8_t) len;
        for (uint32_t i = 0; i < len; i++) out[at++] = data[from + i];
    }
    return at;
}

// The same segment the way the kernels take it: the dictionary by open addressing, the byte count from the number of codes alone, every
// code placed on its own at its closed-form bit position (in the order a stride of `lanes` gives), the framed bytes read back one by
// one.  The bytes are encode_segment's (tests/test_gif_stream.py: the twin runs both).
inline uint32_t encode_segment_pieces(const uint8_t* idx, uint32_t n, bool first, bool last, uint8_t* out, int lanes)
{
    static uint32_t slots[kHashSlots];
    static uint16_t codes[kSegmentPixels];
    static uint32_t words[(kSegmentRoom + 3) / 4 + 2];
    for (int i = 0; i < kHashSlots; i++) slots[i] = Dictionary::kEmpty;
    Dictionary dict = { slots };
    CountCodes count;
    const uint32_t m = match_loop(idx, n, dict, count);            // the counting pass
    const uint32_t data_bytes = segment_data_bytes(m, first, last), bytes = framed_bytes(data_bytes);
    for (int i = 0; i < kHashSlots; i++) slots[i] = Dictionary::kEmpty;
    KeepCodes keep = { codes };
    if (match_loop(idx, n, dict, keep) != m) return 0;             // the storing pass
    uint32_t pad;
    segment_bits(m, first, last, &pad);
    for (size_t i = 0; i < sizeof(words) / sizeof(words[0]); i++) words[i] = 0;
    PlainWords w = { words };
    for (int lane = lanes - 1; lane >= 0; lane--)
        for (uint32_t j = (uint32_t) lane; j < m + 2u + pad; j += (uint32_t) lanes) put_piece(w, codes, m, first, last, j);
    auto data = [&](uint32_t i) { return (unsigned) ((words[i >> 2] >> (8u * (i & 3u))) & 0xFFu); };
    for (uint32_t f = 0; f < bytes; f++) out[f] = (uint8_t) framed_byte(data, data_bytes, f);
    return bytes;
}

// The definition of a frame's unit: into `unit` (room: unit_bound) -> its bytes.  (`pieces`: the segments in the kernels' steps -- the same bytes)
inline size_t encode_frame(const uint8_t* frame, int W, int H, int stride, int flags, int dither, int delay_cs, const uint8_t* lut, uint8_t* unit, Stats* st, bool pieces = false)
{
    const Geometry g = geometry(W, H, stride, flags, dither);
    static DirectTable dict;
    static uint8_t idx[kSegmentPixels];
    lead_bytes(W, H, delay_cs, unit);
    size_t at = kLeadBytes;
    for (uint32_t s = 0; s < g.segments; s++) {
        const uint32_t n = segment_length(g, s);
        for (uint32_t i = 0; i < n; i++) idx[i] = lut[pixel_cell(frame, g, (uint64_t) s * kSegmentPixels + i, true)];
        const bool first = s == 0, last = s + 1 == g.segments;
        at += pieces ? encode_segment_pieces(idx, n, first, last, unit + at, 64) : encode_segment(idx, n, first, last, unit + at, &dict, st);
    }
    unit[at++] = 0x00;
    return at;
}

}  // namespace host

}  // namespace kbe_gif
