// kbe_rows.h -- the project's ONE definition of how the frame filters touch a row of 3-byte pixels in memory: which aligned dwords hold a
// row's bytes and how a run of bytes is cut out of them, how an aligned 16-byte piece of an output row is stored without a byte outside the
// row, and where a tile's row lies in LDS so that its pieces are the row's.  The filters' arithmetic is in their own kbe_*_block.h; this is
// the code around it.  Three compilations read it: hipcc into the kernels (device), hipcc into their entries (host), and g++ into the CPU
// twins -- tests/rows_check.cpp holds it to the bytes themselves, and the serial row walkers of the block headers run on it.
//
// No 3-byte pixel is a byte-wide global access but at a row's two ends:
//   * a row is READ as the aligned dwords that hold a byte of it (fetch_of: a tile's rows into LDS; dword_holds_a_byte: a lane's own run),
//     and a run that starts b = 0..3 bytes into its first dword is cut out by a funnel shift by bytes (realign);
//   * a row is WRITTEN as aligned 16-byte PIECES.  With lead = the row's address modulo 16 the row's bytes are [lead, end) of its pieces;
//     the piece [at, at + 16) is one 16-byte store where it lies inside the row, and dwords and single bytes where one of the row's two
//     ends lies inside it (store_piece).  Nothing outside the row is written, and no two pieces share a byte.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_ROWS_HD __host__ __device__ __forceinline__
#else
#define KBE_ROWS_HD inline
#endif
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace kbe_rows {

constexpr int kMaxSide = 65535;               // of a frame: 3 * kMaxSide bytes of a row and every product of two sides fit 32 bits
constexpr int kPiece = 16;                    // bytes: what one lane stores, and loads from a source
constexpr int kFramesPerLaunch = 12;          // the pointer slots of a launch's arguments, as the encoders' (kbe_units_scan.h)

// -- bytes out of aligned dwords ---------------------------------------------------------------
// the dword that starts b bytes into lo, continued in hi (little endian), 0 <= b <= 3.  On the device this is one instruction, the chip's
// byte-align, by its builtin; the form below it is what that instruction computes, and what a CPU runs
KBE_ROWS_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, b);
#else
    return (uint32_t) ((((uint64_t) hi << 32) | (uint64_t) lo) >> (8u * b));
#endif
}

// the 4 N bytes that start b bytes into the N + 1 dwords x: a funnel shift by bytes.  With b = 0 nothing of x[N] is read
template <int N>
KBE_ROWS_HD void realign(const uint32_t (&x)[N + 1], uint32_t b, uint32_t (&w)[N])
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < N; k++) w[k] = align_bytes(x[k + 1], x[k], b);
}

// Which of the N + 1 ALIGNED dwords around a run of 4 N bytes of a row hold a byte of the row.  The row's bytes are j in [0, row_bytes); the
// bytes wanted are j0 .. j0 + 4 N - 1 (j0 may be negative: an output's piece begins before its row does) and begin b bytes into dword 0;
// dword k covers j0 - b + 4 k .. j0 - b + 4 k + 3.  A dword that holds no byte of the row is not loaded: its address may not exist.
// Nothing is taken from dword N where b = 0.  Int: the caller's own integer, long or int
template <int N, class Int>
KBE_ROWS_HD bool dword_holds_a_byte(Int j0, uint32_t b, int k, Int row_bytes)
{
    const Int first = j0 - (Int) b + 4 * k;
    return first + 3 >= 0 && first < row_bytes && (k < N || b != 0u);
}

// ... and whether all N + 1 do, whatever b is: then a lane loads the first N as 16-byte pieces at dword alignment and the last on its own
template <int N, class Int>
KBE_ROWS_HD bool all_dwords_hold_a_byte(Int j0, Int row_bytes)
{
    return j0 >= 0 && j0 + 4 * N < row_bytes;
}

// -- the piece ---------------------------------------------------------------------------------
// The aligned piece [at, at + 16) of a row's pieces, where the row's bytes are [lead, end) of them: p is 16-byte aligned, and the row's
// bytes in the piece are its bytes [lo, hi)
struct Piece {
    uint8_t* p;
    uint32_t lo, hi;
    KBE_ROWS_HD bool whole() const { return lo == 0u && hi == 16u; }
};

KBE_ROWS_HD Piece piece_of(uint8_t* row, uint32_t lead, uint32_t end, uint32_t at)
{
    return Piece{row - lead + at, at < lead ? lead - at : 0u, end - at < 16u ? end - at : 16u};
}

// which of a piece's four dwords hold a byte of the row: what a lane that reads its piece before it writes it may load
KBE_ROWS_HD bool frame_dword_holds_a_byte(uint32_t d, uint32_t lo, uint32_t hi)
{
    return 4u * d < hi && 4u * d + 4u > lo;
}

// whether all four bytes of a piece's dword d are the row's: stored as a dword then, where the piece is not whole
KBE_ROWS_HD bool dword_is_whole(const Piece& q, uint32_t d)
{
    return q.lo <= 4u * d && 4u * d + 4u <= q.hi;
}

// A piece from its four dwords: 16 bytes at once where it is whole; else every dword that is whole as a dword, and of the others the bytes
// that the row has.  (On a CPU the piece's address is whatever the caller's `lead` makes it: the 16 bytes and the dwords are copied.)
KBE_ROWS_HD void store_piece(const Piece& q, const uint32_t word[4])
{
    if (q.whole()) {
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<uint4*>(q.p) = make_uint4(word[0], word[1], word[2], word[3]);
#else
        memcpy(q.p, word, 16);
#endif
    } else {
        for (uint32_t d = 0; d < 4u; d++) {
            if (dword_is_whole(q, d)) {
#if defined(__HIP_DEVICE_COMPILE__)
                reinterpret_cast<uint32_t*>(q.p)[d] = word[d];
#else
                memcpy(q.p + 4u * d, word + d, 4);
#endif
            } else {
                for (uint32_t b = 4u * d; b < 4u * d + 4u; b++)
                    if (q.lo <= b && b < q.hi) q.p[b] = (uint8_t) (word[d] >> (8u * (b & 3u)));
            }
        }
    }
}

// ... the piece [at, at + 16) of `row`, at < end
KBE_ROWS_HD void store_piece(uint8_t* row, uint32_t lead, uint32_t end, uint32_t at, const uint32_t word[4])
{
    store_piece(piece_of(row, lead, end, at), word);
}

// -- a tile's row ------------------------------------------------------------------------------
// A tile's row of 3 nx bytes is put together in LDS at the global row's own alignment modulo 16 -- lead_of(row) bytes into its LDS row,
// which is 16-byte aligned and 16 bytes longer than the tile's row --, so that the LDS row's aligned pieces are the global row's.
KBE_ROWS_HD uint32_t lead_of(const uint8_t* row)
{
    return (uint32_t) ((uintptr_t) row & 15u);
}

// ... and stored from there: the lane that takes the piece [at, at + 16) of the LDS row, at = 16 * (0, 1, 2, ..)
KBE_ROWS_HD void store_tile_row(const uint8_t* lds_row, uint8_t* row, uint32_t nx, uint32_t at)
{
    const uint32_t lead = lead_of(row), end = lead + 3u * nx;                    // the row's bytes are [lead, end) of the LDS row
    if (at >= end) return;
    uint32_t word[4];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 piece = *reinterpret_cast<const uint4*>(lds_row + at);
    word[0] = piece.x, word[1] = piece.y, word[2] = piece.z, word[3] = piece.w;
#else
    memcpy(word, lds_row + at, 16);
#endif
    store_piece(row, lead, end, at, word);
}

// The aligned dwords that hold a byte of the n pixels of a row that begin at `first`: base[0 .. dwords), every one of which holds a byte of
// the row.  Copied to an aligned place, the row's first pixel lies `shift` bytes into the copy
struct Fetch {
    const uint32_t* base;
    uint32_t shift, dwords;
};

KBE_ROWS_HD uint32_t shift_of(const uint8_t* first)
{
    return (uint32_t) ((uintptr_t) first & 3u);
}

KBE_ROWS_HD Fetch fetch_of(const uint8_t* first, uint32_t n)
{
    const uint32_t shift = (uint32_t) ((uintptr_t) first & 3u), dwords = (shift + 3u * n + 3u) >> 2;
    return Fetch{reinterpret_cast<const uint32_t*>(first - shift), shift, dwords};
}

#if defined(__HIPCC__)
// aligned dwords, loaded and stored as one piece at the alignment of a dword, which the chip's global accesses take
struct __attribute__((packed, aligned(4))) Dwords4 {
    uint32_t x, y, z, w;
};
struct __attribute__((packed, aligned(4))) Dwords3 {
    uint32_t x, y, z;
};
#else
// -- the twins' serial walk --------------------------------------------------------------------
// One row on a CPU, the way the kernels take it: pieces of 16 bytes at the OUTPUT row's alignment (`lead` = its address modulo 16, given by
// the caller so that a test can walk through all sixteen).  piece(at): the piece [at, at + 16); its first byte is byte at - lead of the row
template <class F>
inline void for_each_piece(long row_bytes, uint32_t lead, F&& piece)
{
    for (long at = 0; at < (long) lead + row_bytes; at += kPiece) piece((uint32_t) at);
}

// The N + 1 aligned dwords around the 4 N bytes of `row` that start at its byte j0, b bytes into the first of them, put together byte by
// byte from the row alone -- 0 where the row has no byte or the dword is not loaded --, so nothing outside the row is read
template <int N>
inline void aligned_dwords(const uint8_t* row, long j0, uint32_t b, long row_bytes, uint32_t (&x)[N + 1])
{
    uint8_t bytes[4 * (N + 1)];
    for (long i = 0; i < 4 * (N + 1); i++) {
        const long j = j0 - (long) b + i;
        const bool loaded = all_dwords_hold_a_byte<N>(j0, row_bytes) || dword_holds_a_byte<N>(j0, b, (int) (i / 4), row_bytes);
        bytes[i] = loaded && j >= 0 && j < row_bytes ? row[j] : (uint8_t) 0;
    }
    memcpy(x, bytes, sizeof(bytes));
}
#endif

}  // namespace kbe_rows
