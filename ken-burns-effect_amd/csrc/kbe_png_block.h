// kbe_png_block.h -- the project's ONE definition of the PNG files of the device-side frame writer (kbe_png_encode, include/kbe.h).
// Two compilations read it: hipcc into the kernels of kbe_png.hip, and g++ into tests/png_check.cpp (the CPU twin, whose encode_frame
// below runs the same pieces one after the other).  The device's file is, byte for byte, what encode_frame writes (tests/test_png_gpu.py).
//
// The file: signature, IHDR (8 bits, colour type 2, no interlace), ONE IDAT with one zlib stream (78 01), IEND.  The zlib stream carries
// the FILTERED bytes -- per row the filter byte 1 (Sub), then every byte minus the byte three to its left modulo 256: what
// pipeline.png_bytes compresses -- cut into SEGMENTS of kSegmentBytes (the last one short).  Segments are independent, the unit of work of
// the kernels: no run and no code crosses a boundary.  A segment leaves in one of two forms:
//   coded:  a non-final dynamic-Huffman block (RFC 1951, 3.2.7) followed by an empty stored block (000, padding, 00 00 FF FF), so that
//           the segment ends on a byte boundary;
//   stored: if the coded form is not shorter than a stored block of the same bytes (5 + n), that stored block.
// Behind the last segment: a final empty fixed block (03 00), the Adler-32 of the filtered bytes, the IDAT's CRC-32, IEND.
//
// Tokens (zlib's Z_RLE idea: distance 1 only), in closed form so that any cut of a segment into pieces gives the same tokens: a maximal
// run of n equal bytes is one literal, then (n - 1) / 258 matches of 258 bytes, then the remainder r = (n - 1) % 258 as one more match if
// r >= 3 and as r literals otherwise (token_of).  Codes: per segment a Huffman code over the tokens' literal/length symbols limited to 15
// bits, a code of 7 bits at most over the code lengths (symbols 0..15, 17, 18; 16 is not used), and one bit for each of the distance
// codes 0 and 1 (a complete code; only 0 occurs).  All of it integer arithmetic, the same function on both sides (lengths_from_order).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_PNG_HD __host__ __device__ __forceinline__
#else
#define KBE_PNG_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

namespace kbe_png {

constexpr int kSegmentBytes = 16384;    // 4096..65535 (a stored block's limit); 512^2 photo-like: 0.888 of zlib level 1's bytes (8 KB: 0.891, 32 KB: 0.886)
constexpr int kFlagBgr = 1;             // KBE_PNG_BGR: the frames hold B, G, R
constexpr int kLeadBytes = 43;          // signature 8, IHDR 25, the IDAT's length and tag 8, the zlib header 2: in front of a frame's first segment
constexpr int kTailBytes = 22;          // the final fixed block 2, Adler-32 4, the IDAT's CRC 4, IEND 12: behind its last one
constexpr int kLitSyms = 286, kClSyms = 19, kLitLimit = 15, kClLimit = 7;
constexpr int kEob = 256;
constexpr uint32_t kAdlerMod = 65521u, kCrcPoly = 0xEDB88320u;
static_assert(kSegmentBytes >= 4096 && kSegmentBytes <= 65535, "a stored block holds at most 65535 bytes");

struct Geometry {
    int W, H, stride, bgr;
    uint32_t row_bytes;         // 1 + 3 W
    uint64_t raw;               // filtered bytes of a frame
    uint32_t segments;
};

KBE_PNG_HD Geometry geometry(int W, int H, int stride, int flags)
{
    Geometry g;
    g.W = W; g.H = H; g.stride = stride; g.bgr = (flags & kFlagBgr) != 0;
    g.row_bytes = 1u + 3u * (uint32_t) W;
    g.raw = (uint64_t) H * g.row_bytes;
    g.segments = (uint32_t) ((g.raw + kSegmentBytes - 1) / kSegmentBytes);
    return g;
}

// bytes that hold ANY W x H frame's file: every segment stored.  0: a size the encoder refuses (the file would not stay below 2^31 bytes)
KBE_PNG_HD size_t file_bound(int W, int H)
{
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return 0;
    const Geometry g = geometry(W, H, 0, 0);
    const uint64_t bound = (uint64_t) kLeadBytes + kTailBytes + g.raw + 5ull * g.segments;
    return bound < (1ull << 31) ? (size_t) bound : 0;
}

KBE_PNG_HD uint32_t segment_length(const Geometry& g, uint32_t segment)
{
    const uint64_t left = g.raw - (uint64_t) segment * kSegmentBytes;
    return left < (uint64_t) kSegmentBytes ? (uint32_t) left : (uint32_t) kSegmentBytes;
}

// byte `at` (< g.raw) of a frame's filtered stream
KBE_PNG_HD unsigned filtered_byte(const uint8_t* frame, const Geometry& g, uint32_t at)
{
    const uint32_t row = at / g.row_bytes, c = at - row * g.row_bytes;
    if (c == 0) return 1u;
    const uint32_t x = (c - 1) / 3u, ch = (c - 1) - 3u * x;
    const uint8_t* p = frame + (size_t) row * (size_t) g.stride + 3 * (size_t) x + (g.bgr ? 2u - ch : ch);
    return ((unsigned) p[0] - (x ? (unsigned) p[-3] : 0u)) & 0xFFu;
}

// ---------------------------------------------------------------------------------------
// tokens
// ---------------------------------------------------------------------------------------
// what leaves at byte k of a maximal run of n equal bytes: 0 nothing (the byte lies inside a match), 1 the byte as a literal, L >= 3 a match
// of length L at distance 1
KBE_PNG_HD int token_of(uint32_t k, uint32_t n)
{
    if (k == 0) return 1;
    const uint32_t m = n - 1, j = k - 1, q = j / 258u, at = j - q * 258u, full = m / 258u, r = m - full * 258u;
    if (q < full) return at == 0 ? 258 : 0;
    if (r >= 3) return at == 0 ? (int) r : 0;
    return 1;
}

// a match length 3..258 as its symbol 257..285 and extra bits (RFC 1951, 3.2.5)
KBE_PNG_HD void length_symbol(int L, int* sym, int* extra_bits, unsigned* extra)
{
    const unsigned l = (unsigned) L - 3u;
    if (L == 258) { *sym = 285; *extra_bits = 0; *extra = 0; return; }
    if (l < 8) { *sym = 257 + (int) l; *extra_bits = 0; *extra = 0; return; }
    const int eb = (31 - __builtin_clz(l)) - 2;
    *sym = 257 + 4 * (eb + 1) + (int) ((l >> eb) & 3u);
    *extra_bits = eb;
    *extra = l & ((1u << eb) - 1u);
}

// The tokens of bytes [begin, end) of a segment b[0 .. n): `start` is where the run that holds byte `begin` starts, `next` where the first
// run at or behind `end` starts (n if there is none).  out(kind, byte): token_of's result for every byte in order.  The twin walks a
// segment in one piece (0, n, 0, n); a lane of the kernels walks its own piece with what two scans across the workgroup told it.
template <class Out>
KBE_PNG_HD void walk(const uint8_t* b, int begin, int end, int start, int next, Out& out)
{
    int i = begin, s = start;
    while (i < end) {
        int e = i + 1;
        while (e < end && b[e] == b[e - 1]) e++;
        const uint32_t n = (uint32_t) ((e < end ? e : next) - s);
        for (int p = i; p < e; p++) out.token(token_of((uint32_t) (p - s), n), b[p]);
        i = e;
        s = e;
    }
}

// ---------------------------------------------------------------------------------------
// codes
// ---------------------------------------------------------------------------------------
// everything a segment's code construction touches: in LDS in the kernels, on the stack in the twin
struct Work {
    uint32_t hist[kLitSyms];
    uint32_t weight[kLitSyms];          // the tree's inner nodes
    uint16_t up[2 * kLitSyms];          // a node's parent, then its depth
    uint16_t order[kLitSyms];           // the used symbols by (count, symbol)
    uint16_t lit_code[kLitSyms];        // codes with their bits reversed: as they enter the stream
    uint8_t lit_len[kLitSyms];
    uint32_t cl_hist[kClSyms];
    uint16_t cl_code[kClSyms];
    uint8_t cl_len[kClSyms];
    uint8_t seq_sym[kLitSyms + 2], seq_extra[kLitSyms + 2];     // the code lengths as symbols 0..15, 17, 18
    uint32_t count[kLitLimit + 2], next[kLitLimit + 2];         // codes per length, the next code of a length
    int used, limited;
};

// place of symbol i among the used symbols in the order (count, symbol); the kernels take one symbol per lane
KBE_PNG_HD int rank_of(const uint32_t* hist, int nsym, int i)
{
    int rank = 0;
    for (int j = 0; j < nsym; j++) rank += hist[j] && (hist[j] < hist[i] || (hist[j] == hist[i] && j < i)) ? 1 : 0;
    return rank;
}

// -> the number of used symbols
KBE_PNG_HD int order_symbols(const uint32_t* hist, int nsym, uint16_t* order)
{
    int used = 0;
    for (int i = 0; i < nsym; i++)
        if (hist[i]) { order[rank_of(hist, nsym, i)] = (uint16_t) i; used++; }
    return used;
}

// Code lengths of at most `limit` bits for the `used` symbols of order[] (counts hist[], their sum below 2^32), 0 for all others.  A
// Huffman tree by the two-queue method (ties: the leaf first), its depths counted per length; depths beyond the limit are folded into it and
// the Kraft sum is brought back to exactly 1 by moving one code at a time a level down; the lengths then go to the symbols in order, the
// rarest the longest.  One used symbol: length 1 (the one code that is not complete).  -> 1 if the limit cut the tree
KBE_PNG_HD int lengths_from_order(const uint32_t* hist, const uint16_t* order, int used, int nsym, int limit, uint8_t* len, uint32_t* weight, uint16_t* up, uint32_t* count)
{
    for (int i = 0; i < nsym; i++) len[i] = 0;
    if (used == 0) return 0;
    if (used == 1) { len[order[0]] = 1; return 0; }
    // nodes 0 .. used-1: the leaves in order; used .. 2 used - 2: inner nodes in the order they are made (their weights do not decrease)
    int leaf = 0, inner = used;
    for (int made = used; made < 2 * used - 1; made++) {
        uint32_t w = 0;
        for (int k = 0; k < 2; k++) {
            const bool take_leaf = leaf < used && (inner >= made || hist[order[leaf]] <= weight[inner - used]);
            if (take_leaf) { w += hist[order[leaf]]; up[leaf++] = (uint16_t) made; }
            else { w += weight[inner - used]; up[inner++] = (uint16_t) made; }
        }
        weight[made - used] = w;
    }
    for (int l = 0; l <= limit; l++) count[l] = 0;
    int limited = 0;
    up[2 * used - 2] = 0;
    for (int node = 2 * used - 3; node >= 0; node--) {
        const int depth = up[up[node]] + 1;
        up[node] = (uint16_t) depth;
        if (node < used) {
            if (depth > limit) limited = 1;
            count[depth < limit ? depth : limit]++;
        }
    }
    uint32_t kraft = 0;
    for (int l = 1; l <= limit; l++) kraft += count[l] << (limit - l);
    while (kraft > (1u << limit)) {
        count[limit]--;
        for (int l = limit - 1; l >= 1; l--)
            if (count[l]) { count[l]--; count[l + 1] += 2; break; }
        kraft--;
    }
    int k = 0;
    for (int l = limit; l >= 1; l--)
        for (uint32_t c = 0; c < count[l]; c++) len[order[k++]] = (uint8_t) l;
    return limited;
}

// canonical codes (RFC 1951, 3.2.2) of the lengths, bits reversed: the stream takes Huffman codes from their most significant bit
KBE_PNG_HD void canonical_codes(const uint8_t* len, int nsym, int limit, uint16_t* code, uint32_t* count, uint32_t* next)
{
    for (int l = 0; l <= limit; l++) count[l] = 0;
    for (int i = 0; i < nsym; i++) count[len[i]]++;
    count[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l <= limit; l++) { c = (c + count[l - 1]) << 1; next[l] = c; }
    for (int i = 0; i < nsym; i++) {
        const int l = len[i];
        uint32_t v = l ? next[l]++ : 0u, r = 0;
        for (int k = 0; k < l; k++) { r = (r << 1) | (v & 1u); v >>= 1; }
        code[i] = (uint16_t) r;
    }
}

struct CountBits {
    uint32_t n;
    KBE_PNG_HD void bits(uint32_t, int len) { n += (uint32_t) len; }
};

// A coded segment's block header through out.bits(value, length <= 16), least significant bit first: BFINAL 0, BTYPE 2, HLIT, HDIST = 2
// codes, HCLEN, the code-length code, the lengths.  Builds the code-length code in `w` (w->lit_len holds the lengths).  Zero runs: 18 for
// 11..138 at a time while 11 or more are left, then 17 for 3..10, then single zeros.
template <class Bits>
KBE_PNG_HD void block_header(Work* w, Bits& out)
{
    int nlit = kLitSyms;
    while (nlit > 257 && w->lit_len[nlit - 1] == 0) nlit--;
    int ns = 0;
    for (int i = 0; i < kClSyms; i++) w->cl_hist[i] = 0;
    for (int i = 0; i < nlit + 2;) {
        const int l = i < nlit ? w->lit_len[i] : 1;                 // (the two distance codes: one bit each)
        if (l) { w->seq_sym[ns] = (uint8_t) l; w->seq_extra[ns++] = 0; w->cl_hist[l]++; i++; continue; }
        int z = 1;
        while (i + z < nlit && w->lit_len[i + z] == 0) z++;
        i += z;
        while (z >= 11) { const int t = z < 138 ? z : 138; w->seq_sym[ns] = 18; w->seq_extra[ns++] = (uint8_t) (t - 11); w->cl_hist[18]++; z -= t; }
        if (z >= 3) { w->seq_sym[ns] = 17; w->seq_extra[ns++] = (uint8_t) (z - 3); w->cl_hist[17]++; z = 0; }
        for (; z > 0; z--) { w->seq_sym[ns] = 0; w->seq_extra[ns++] = 0; w->cl_hist[0]++; }
    }
    const int used = order_symbols(w->cl_hist, kClSyms, w->order);
    w->limited |= lengths_from_order(w->cl_hist, w->order, used, kClSyms, kClLimit, w->cl_len, w->weight, w->up, w->count) << 1;
    canonical_codes(w->cl_len, kClSyms, kClLimit, w->cl_code, w->count, w->next);
    const uint8_t cl_order[kClSyms] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    int ncl = kClSyms;
    while (ncl > 4 && w->cl_len[cl_order[ncl - 1]] == 0) ncl--;
    out.bits(0u, 1);
    out.bits(2u, 2);
    out.bits((uint32_t) (nlit - 257), 5);
    out.bits(1u, 5);
    out.bits((uint32_t) (ncl - 4), 4);
    for (int i = 0; i < ncl; i++) out.bits(w->cl_len[cl_order[i]], 3);
    for (int i = 0; i < ns; i++) {
        const int s = w->seq_sym[i];
        out.bits(w->cl_code[s], w->cl_len[s]);
        if (s == 17) out.bits(w->seq_extra[i], 3);
        if (s == 18) out.bits(w->seq_extra[i], 7);
    }
}

// a token's bits: a literal's code; a match's length code, extra bits and the distance code 0 (one bit)
KBE_PNG_HD int token_bits(const Work* w, int kind, unsigned byte, uint32_t* value)
{
    if (kind == 1) { *value = w->lit_code[byte]; return w->lit_len[byte]; }
    int sym, eb;
    unsigned extra;
    length_symbol(kind, &sym, &eb, &extra);
    const int l = w->lit_len[sym];
    *value = (uint32_t) w->lit_code[sym] | (extra << l);
    return l + eb + 1;
}

struct HistogramOut {
    uint32_t* hist;
    KBE_PNG_HD void token(int kind, unsigned byte)
    {
        if (kind == 1) hist[byte]++;
        else if (kind) { int sym, eb; unsigned extra; length_symbol(kind, &sym, &eb, &extra); hist[sym]++; }
    }
};

struct LengthOut {
    const Work* w;
    uint32_t n;
    KBE_PNG_HD void token(int kind, unsigned byte)
    {
        uint32_t v;
        if (kind) n += (uint32_t) token_bits(w, kind, byte, &v);
    }
};

template <class Bits>
struct PackOut {
    const Work* w;
    Bits& out;
    KBE_PNG_HD void token(int kind, unsigned byte)
    {
        uint32_t v;
        if (kind) { const int l = token_bits(w, kind, byte, &v); out.bits(v, l); }
    }
};

// bits into zeroed 32-bit words from bit `at` on, least significant bit first, the way the kernels pack them: whole words leave through
// words.merge(index, value) -- an OR, atomic in LDS, because the first and the last word of a lane's bits are also its neighbours'
template <class Words>
struct WordBits {
    Words words;
    uint64_t acc;
    int n;
    uint32_t word;
    KBE_PNG_HD void start(uint32_t at) { acc = 0; n = (int) (at & 31u); word = at >> 5; }
    KBE_PNG_HD void bits(uint32_t v, int len)
    {
        acc |= (uint64_t) v << n;
        n += len;
        if (n >= 32) { words.merge(word++, (uint32_t) acc); acc >>= 32; n -= 32; }
    }
    KBE_PNG_HD void finish() { if (n && (uint32_t) acc) words.merge(word, (uint32_t) acc); }
    KBE_PNG_HD uint32_t position() const { return word * 32u + (uint32_t) n; }
};

// bytes of the coded form of a segment whose header takes header_bits and whose tokens take token_bits: EOB, the empty stored block
KBE_PNG_HD uint32_t coded_bytes(const Work* w, uint32_t header_bits, uint32_t tokens_bits)
{
    return (header_bits + tokens_bits + w->lit_len[kEob] + 3u + 7u) / 8u + 4u;
}

// behind the last token: EOB, then the empty stored block that restores the byte boundary (000, padding, LEN 0, NLEN FFFF)
template <class Bits>
KBE_PNG_HD void end_coded(const Work* w, Bits& out, uint32_t bits_so_far)
{
    out.bits(w->lit_code[kEob], w->lit_len[kEob]);
    out.bits(0u, 3);
    const uint32_t at = (bits_so_far + w->lit_len[kEob] + 3u) & 7u;
    if (at) out.bits(0u, (int) (8u - at));
    out.bits(0u, 16);
    out.bits(0xFFFFu, 16);
}

// ---------------------------------------------------------------------------------------
// check sums.  Adler-32 of N bytes b[i]: A = 1 + sum b[i], B = N + sum (N - i) b[i], both mod 65521: a piece [p, q) contributes
// a = sum b[i] and (N - q) a + sum (q - i) b[i], whatever the other pieces hold.
// CRC-32 (reflected, polynomial EDB88320): raw(M) = the register after M from 0, without the final inversion, is linear, so
// raw(M1 M2) = raw(M1) x^(8 |M2|) + raw(M2) and crc(M) = raw(M) + FFFFFFFF x^(8 |M|) + FFFFFFFF: every piece is advanced by the bytes
// behind it with the constants x^(8 2^k) mod P (Powers::x8, built on the host) and the pieces are XORed.
// ---------------------------------------------------------------------------------------
KBE_PNG_HD uint32_t gf_multiply(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

struct Powers { uint32_t x8[32]; };     // x^(8 2^k) mod P

KBE_PNG_HD uint32_t crc_advance(const uint32_t* x8, uint32_t crc, uint64_t bytes)
{
    for (int k = 0; bytes; k++, bytes >>= 1)
        if (bytes & 1u) crc = gf_multiply(x8[k & 31], crc);
    return crc;
}

KBE_PNG_HD uint32_t crc_table_entry(unsigned i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
    return c;
}

KBE_PNG_HD uint32_t crc_raw(const uint32_t* table, const uint8_t* p, uint32_t n)
{
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c;
}

// what the bytes p[0 .. n) of a frame's filtered stream, `behind` bytes of the stream behind them, add to A and to B
KBE_PNG_HD void adler_piece(const uint8_t* p, uint32_t n, uint64_t behind, uint32_t* a, uint32_t* b)
{
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = 0; i < n; i++) { sa += p[i]; sb += (uint64_t) (n - i) * p[i]; }
    *a = (uint32_t) (sa % kAdlerMod);
    *b = (uint32_t) (((behind % kAdlerMod) * (sa % kAdlerMod) + sb) % kAdlerMod);
}

// the frame's last 22 bytes from the sums over its pieces (sum_a, sum_b: mod 65521 or not), the XOR of the segments' advanced raw CRCs, and
// the file's size
KBE_PNG_HD void tail_bytes(const uint32_t* x8, const uint32_t* table, uint64_t raw, uint64_t sum_a, uint64_t sum_b, uint32_t crc_segments, uint64_t file_bytes, uint8_t* out)
{
    const uint32_t A = (uint32_t) ((1u + sum_a) % kAdlerMod), B = (uint32_t) ((raw + sum_b) % kAdlerMod);
    const uint64_t covered = file_bytes - 57u + 4u;             // the IDAT's tag and data
    out[0] = 0x03; out[1] = 0x00;
    out[2] = (uint8_t) (B >> 8); out[3] = (uint8_t) B; out[4] = (uint8_t) (A >> 8); out[5] = (uint8_t) A;
    const uint8_t front[6] = { 'I', 'D', 'A', 'T', 0x78, 0x01 };
    uint32_t crc = crc_segments ^ crc_advance(x8, crc_raw(table, front, 6), covered - 6) ^ crc_raw(table, out, 6) ^ crc_advance(x8, 0xFFFFFFFFu, covered) ^ 0xFFFFFFFFu;
    out[6] = (uint8_t) (crc >> 24); out[7] = (uint8_t) (crc >> 16); out[8] = (uint8_t) (crc >> 8); out[9] = (uint8_t) crc;
    const uint8_t iend[12] = { 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82 };
    for (int i = 0; i < 12; i++) out[10 + i] = iend[i];
}

// the IDAT's length into a frame's first 43 bytes
KBE_PNG_HD void lead_length(uint8_t* lead, uint64_t file_bytes)
{
    const uint32_t d = (uint32_t) (file_bytes - 57u);
    lead[33] = (uint8_t) (d >> 24); lead[34] = (uint8_t) (d >> 16); lead[35] = (uint8_t) (d >> 8); lead[36] = (uint8_t) d;
}

// ---------------------------------------------------------------------------------------
// host side: the constants, and the definition of a frame's file
// ---------------------------------------------------------------------------------------
namespace host {

struct Tables {
    Powers pw;
    uint32_t crc[256];
    uint8_t lead[kLeadBytes + 1];       // (the IDAT's length is filled in per frame: lead_length)
};

inline void tables_build(int W, int H, Tables* t)
{
    for (unsigned i = 0; i < 256; i++) t->crc[i] = crc_table_entry(i);
    uint32_t p = 1u << 23;                                  // x^8
    for (int k = 0; k < 32; k++) { t->pw.x8[k] = p; p = gf_multiply(p, p); }
    const uint8_t head[16] = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R' };
    uint8_t* l = t->lead;
    for (int i = 0; i < 16; i++) l[i] = head[i];
    l[16] = (uint8_t) ((unsigned) W >> 24); l[17] = (uint8_t) (W >> 16); l[18] = (uint8_t) (W >> 8); l[19] = (uint8_t) W;
    l[20] = (uint8_t) ((unsigned) H >> 24); l[21] = (uint8_t) (H >> 16); l[22] = (uint8_t) (H >> 8); l[23] = (uint8_t) H;
    l[24] = 8; l[25] = 2; l[26] = 0; l[27] = 0; l[28] = 0;
    const uint32_t c = crc_advance(t->pw.x8, 0xFFFFFFFFu, 17) ^ crc_raw(t->crc, l + 12, 17) ^ 0xFFFFFFFFu;
    l[29] = (uint8_t) (c >> 24); l[30] = (uint8_t) (c >> 16); l[31] = (uint8_t) (c >> 8); l[32] = (uint8_t) c;
    l[33] = l[34] = l[35] = l[36] = 0;
    l[37] = 'I'; l[38] = 'D'; l[39] = 'A'; l[40] = 'T'; l[41] = 0x78; l[42] = 0x01; l[43] = 0;
}

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
};

struct Stats { long coded, stored, limited_lit, limited_cl; };

// one segment b[0 .. n) into out (room: n + 5) -> its bytes
inline uint32_t encode_segment(const uint8_t* b, uint32_t n, uint8_t* out, Work* w, Stats* st)
{
    for (int i = 0; i < kLitSyms; i++) w->hist[i] = 0;
    HistogramOut h = { w->hist };
    walk(b, 0, (int) n, 0, (int) n, h);
    w->hist[kEob] = 1;
    w->used = order_symbols(w->hist, kLitSyms, w->order);
    w->limited = lengths_from_order(w->hist, w->order, w->used, kLitSyms, kLitLimit, w->lit_len, w->weight, w->up, w->count);
    canonical_codes(w->lit_len, kLitSyms, kLitLimit, w->lit_code, w->count, w->next);
    CountBits header = { 0 };
    block_header(w, header);
    LengthOut lengths = { w, 0 };
    walk(b, 0, (int) n, 0, (int) n, lengths);
    const uint32_t coded = coded_bytes(w, header.n, lengths.n);
    if (st) { st->limited_lit += w->limited & 1; st->limited_cl += (w->limited >> 1) & 1; }
    if (coded >= n + 5) {
        if (st) st->stored++;
        out[0] = 0; out[1] = (uint8_t) n; out[2] = (uint8_t) (n >> 8); out[3] = (uint8_t) ~n; out[4] = (uint8_t) (~n >> 8);
        for (uint32_t i = 0; i < n; i++) out[5 + i] = b[i];
        return n + 5;
    }
    if (st) st->coded++;
    ByteBits bits = { out, 0, 0, 0 };
    block_header(w, bits);
    PackOut<ByteBits> pack = { w, bits };
    walk(b, 0, (int) n, 0, (int) n, pack);
    end_coded(w, bits, header.n + lengths.n);
    return bits.count;                  // (== coded)
}

// The same segment the way the kernels take it: in pieces of `piece` bytes, every piece told by its neighbours where the run that reaches
// into it starts and where the run that leaves it ends, its bits packed at their place into words (WordBits).  The bytes are
// encode_segment's (tests/test_png_stream.py: the twin runs both).  out: room for n + 5 bytes rounded up to words, plus a word.
struct PlainWords {
    uint32_t* w;
    void merge(uint32_t index, uint32_t value) { w[index] |= value; }
};

inline uint32_t encode_segment_pieces(const uint8_t* b, uint32_t n, uint8_t* out, Work* w, int piece)
{
    const int pieces = ((int) n + piece - 1) / piece;
    int* start = new int[pieces];
    int* next = new int[pieces];
    uint32_t* bits = new uint32_t[pieces];
    for (int k = 0, last = 0; k < pieces; k++) {                        // (what the kernels' two scans give)
        const int begin = k * piece;
        start[k] = begin == 0 || b[begin] != b[begin - 1] ? begin : last;
        for (int p = begin; p < begin + piece && p < (int) n; p++)
            if (p == 0 || b[p] != b[p - 1]) last = p;
    }
    for (int k = pieces - 1, first = (int) n; k >= 0; k--) {
        next[k] = first;
        for (int p = ((k + 1) * piece < (int) n ? (k + 1) * piece : (int) n) - 1; p >= k * piece; p--)
            if (p == 0 || b[p] != b[p - 1]) first = p;
    }
    auto end_of = [&](int k) { return (k + 1) * piece < (int) n ? (k + 1) * piece : (int) n; };
    for (int i = 0; i < kLitSyms; i++) w->hist[i] = 0;
    HistogramOut h = { w->hist };
    for (int k = 0; k < pieces; k++) walk(b, k * piece, end_of(k), start[k], next[k], h);
    w->hist[kEob] = 1;
    w->used = order_symbols(w->hist, kLitSyms, w->order);
    w->limited = lengths_from_order(w->hist, w->order, w->used, kLitSyms, kLitLimit, w->lit_len, w->weight, w->up, w->count);
    canonical_codes(w->lit_len, kLitSyms, kLitLimit, w->lit_code, w->count, w->next);
    const uint32_t words = (n + 5 + 3) / 4 + 1;
    uint32_t* packed = new uint32_t[words > 256 ? words : 256]();
    WordBits<PlainWords> header = { { packed }, 0, 0, 0 };
    header.start(0);
    block_header(w, header);
    header.finish();
    const uint32_t header_bits = header.position();
    uint32_t tokens_bits = 0;
    for (int k = 0; k < pieces; k++) {
        LengthOut lengths = { w, 0 };
        walk(b, k * piece, end_of(k), start[k], next[k], lengths);
        bits[k] = tokens_bits;
        tokens_bits += lengths.n;
    }
    uint32_t size = coded_bytes(w, header_bits, tokens_bits);
    if (size >= n + 5) {
        size = n + 5;
        out[0] = 0; out[1] = (uint8_t) n; out[2] = (uint8_t) (n >> 8); out[3] = (uint8_t) ~n; out[4] = (uint8_t) (~n >> 8);
        for (uint32_t i = 0; i < n; i++) out[5 + i] = b[i];
    } else {
        for (int k = pieces - 1; k >= 0; k--) {                         // (in any order)
            WordBits<PlainWords> mine = { { packed }, 0, 0, 0 };
            mine.start(header_bits + bits[k]);
            PackOut<WordBits<PlainWords> > pack = { w, mine };
            walk(b, k * piece, end_of(k), start[k], next[k], pack);
            mine.finish();
        }
        WordBits<PlainWords> last = { { packed }, 0, 0, 0 };
        last.start(header_bits + tokens_bits);
        end_coded(w, last, header_bits + tokens_bits);
        last.finish();
        for (uint32_t i = 0; i < size; i++) out[i] = (uint8_t) (packed[i >> 2] >> (8 * (i & 3)));
    }
    delete[] start; delete[] next; delete[] bits; delete[] packed;
    return size;
}

// The definition of a frame's file: into `file` (room: file_bound) -> its bytes.  (`piece`: the segments in the kernels' steps -- the same bytes)
inline size_t encode_frame(const uint8_t* frame, int W, int H, int stride, int flags, const Tables& t, uint8_t* file, Stats* st, int piece = 0)
{
    const Geometry g = geometry(W, H, stride, flags);
    static Work w;
    static uint8_t b[kSegmentBytes];
    size_t at = kLeadBytes;
    // the segments' bytes and Adler sums first: their CRCs are advanced by what lies behind them, which needs the file's size
    uint32_t* sizes = new uint32_t[g.segments];
    uint64_t sum_a = 0, sum_b = 0;
    for (uint32_t s = 0; s < g.segments; s++) {
        const uint32_t n = segment_length(g, s);
        for (uint32_t i = 0; i < n; i++) b[i] = (uint8_t) filtered_byte(frame, g, s * (uint32_t) kSegmentBytes + i);
        uint32_t a, c;
        adler_piece(b, n, g.raw - ((uint64_t) s * kSegmentBytes + n), &a, &c);
        sum_a += a; sum_b += c;
        at += sizes[s] = piece ? encode_segment_pieces(b, n, file + at, &w, piece) : encode_segment(b, n, file + at, &w, st);
    }
    const size_t total = at + kTailBytes;
    uint32_t crc = 0;
    size_t pos = kLeadBytes;
    for (uint32_t s = 0; s < g.segments; pos += sizes[s++]) crc ^= crc_advance(t.pw.x8, crc_raw(t.crc, file + pos, sizes[s]), (uint64_t) (total - 16) - (pos + sizes[s]));
    delete[] sizes;
    for (int i = 0; i < kLeadBytes; i++) file[i] = t.lead[i];
    lead_length(file, total);
    tail_bytes(t.pw.x8, t.crc, g.raw, sum_a, sum_b, crc, total, file + at);
    return total;
}

}  // namespace host

}  // namespace kbe_png
