// kbe_shutter_block.h -- the project's ONE definition of the shutter mean of kbe_shutter_mean_u8 (include/kbe_shutter.h).  Two compilations
// read it: hipcc into the kernel of kbe_shutter.hip, and g++ into tests/shutter_check.cpp, which holds the packed forms below to the plain
// one on every input they can meet and runs the rows serially.  The device's bytes are what mean_row below gives (tests/test_shutter_gpu.py,
// through the NumPy twin).
//
// One output frame is the mean of S source frames ("samples"), byte by byte, 1 <= S <= kMaxSamples = 32.  For every byte position
//     sum = the sum of the S source bytes                     (at most 255 * 32 = 8160)
//     out = (2 sum + S) / (2 S)                               (integer division: the mean, rounded half up; 2 sum + S <= 16352)
// Channels are not looked at: a row is 3 W bytes.  S = 1 copies.  The same source may appear more than once among the S.  No floating point.
//
// The packed forms, which the kernel uses instead of the plain one (and which are the plain one: shutter_check brute):
//   * a row is taken in PIECES of 16 bytes, four dwords.  The sums of a piece are kept as two 16-bit lanes per dword: the even bytes of dword d
//     in Acc::even[d], the odd bytes in Acc::odd[d] (add).  A lane holds at most 8160: no carry leaves it.
//   * the division is a multiply-high: with d = 2 S and M = ceil(2^32 / d) (magic), floor(t M / 2^32) = floor(t / d) for every t < 2^32 / d,
//     since 0 <= M d - 2^32 < d; t is at most 16352 here (finish).
//   * a piece of a source starts anywhere: its 16 bytes are cut out of the five ALIGNED dwords x[0..4] that hold them, b = 0..3 bytes into
//     x[0]: w[k] = the dword at byte 4 k + b of x (realign: a funnel shift by bytes).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_SHUTTER_HD __host__ __device__ __forceinline__
#else
#define KBE_SHUTTER_HD inline
#endif
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace kbe_shutter {

constexpr int kMaxSide = 65535;
constexpr int kMaxSamples = 32;
constexpr int kPiece = 16;                    // bytes: what one lane of the kernel loads from a source, and stores

// the plain form: the mean of S bytes that add up to sum, rounded half up
KBE_SHUTTER_HD uint32_t mean_of(uint32_t sum, uint32_t S)
{
    return (2u * sum + S) / (2u * S);
}

// M = ceil(2^32 / (2 S)); 2 S >= 2, so it fits 32 bits
KBE_SHUTTER_HD uint32_t magic(uint32_t S)
{
    return 0xFFFFFFFFu / (2u * S) + 1u;
}

KBE_SHUTTER_HD uint32_t mul_hi(uint32_t a, uint32_t b)
{
    return (uint32_t) (((uint64_t) a * (uint64_t) b) >> 32);
}

// the mean of one 16-bit lane by the multiply-high: mean_of(sum, S) for every sum <= 255 S, M = magic(S)
KBE_SHUTTER_HD uint32_t mean_by_magic(uint32_t sum, uint32_t S, uint32_t M)
{
    return mul_hi(2u * sum + S, M);
}

// the sums of one piece: two 16-bit lanes per dword
struct Acc {
    uint32_t even[4], odd[4];
};

KBE_SHUTTER_HD void clear(Acc& a)
{
    for (int d = 0; d < 4; d++) a.even[d] = a.odd[d] = 0u;
}

KBE_SHUTTER_HD void add(Acc& a, const uint32_t w[4])
{
    for (int d = 0; d < 4; d++) {
        a.even[d] += w[d] & 0x00FF00FFu;
        a.odd[d] += (w[d] >> 8) & 0x00FF00FFu;
    }
}

// the four output dwords of a piece from its sums
KBE_SHUTTER_HD void finish(const Acc& a, uint32_t S, uint32_t M, uint32_t out[4])
{
    for (int d = 0; d < 4; d++) {
        const uint32_t b0 = mean_by_magic(a.even[d] & 0xFFFFu, S, M), b1 = mean_by_magic(a.odd[d] & 0xFFFFu, S, M);
        const uint32_t b2 = mean_by_magic(a.even[d] >> 16, S, M), b3 = mean_by_magic(a.odd[d] >> 16, S, M);
        out[d] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
}

// the dword that starts b bytes into lo, continued in hi (little endian), 0 <= b <= 3.  On the device this is one instruction, the chip's
// byte-align, by its builtin; the form below it is what that instruction computes, and what a CPU runs
KBE_SHUTTER_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, b);
#else
    return (uint32_t) ((((uint64_t) hi << 32) | (uint64_t) lo) >> (8u * b));
#endif
}

// the 16 bytes that start b bytes into the 20 bytes x[0..4]: a funnel shift by bytes.  With b = 0 nothing of x[4] is read
KBE_SHUTTER_HD void realign(const uint32_t x[5], uint32_t b, uint32_t w[4])
{
    for (int k = 0; k < 4; k++) w[k] = align_bytes(x[k + 1], x[k], b);
}

// Which of the five ALIGNED dwords around a source's 16 bytes hold a byte of the row.  The row's bytes are j in [0, row_bytes); the 16 bytes
// wanted are j0 .. j0 + 15 (j0 may be negative: the output's piece begins before its row does) and begin b bytes into dword 0; dword k covers
// j0 - b + 4 k .. j0 - b + 4 k + 3.  A dword that holds no byte of the row is not loaded: its address may not exist.  Nothing is taken from
// dword 4 where b = 0.
KBE_SHUTTER_HD bool dword_holds_a_byte(long j0, uint32_t b, int k, long row_bytes)
{
    const long first = j0 - (long) b + 4 * k;
    return first + 3 >= 0 && first < row_bytes && (k < 4 || b != 0u);
}

// ... and whether all five do, whatever b is: then a lane loads them as one 16-byte piece at dword alignment and one dword
KBE_SHUTTER_HD bool all_dwords_hold_a_byte(long j0, long row_bytes)
{
    return j0 >= 0 && j0 + 16 < row_bytes;
}

#if !defined(__HIPCC__)
// One output row on a CPU, serially, the way the kernel takes it: pieces of 16 bytes at the OUTPUT row's alignment (`lead` = its address
// modulo 16, given by the caller so that a test can walk through all sixteen), every source realigned by its own address modulo 4
// (row_class[s]: the address of the source row's first byte, any number congruent to it modulo 4).  The aligned dwords are put together byte
// by byte from the row alone -- 0 where the row has no byte or the dword is not loaded --, so nothing outside a row is read.
inline void mean_row(const uint8_t* const* rows, const uint32_t* row_class, uint32_t S, long row_bytes, uint32_t lead, uint8_t* out)
{
    const uint32_t M = magic(S);
    for (long at = 0; at < (long) lead + row_bytes; at += kPiece) {
        const long j0 = at - (long) lead;
        Acc acc;
        clear(acc);
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t b = (uint32_t) (((long) row_class[s] + j0) & 3);
            uint8_t bytes[20];
            for (long i = 0; i < 20; i++) {
                const long j = j0 - (long) b + i;
                const bool loaded = all_dwords_hold_a_byte(j0, row_bytes) || dword_holds_a_byte(j0, b, (int) (i / 4), row_bytes);
                bytes[i] = loaded && j >= 0 && j < row_bytes ? rows[s][j] : (uint8_t) 0;
            }
            uint32_t x[5], w[4];
            memcpy(x, bytes, 20);
            realign(x, b, w);
            add(acc, w);
        }
        uint32_t word[4];
        uint8_t piece[16];
        finish(acc, S, M, word);
        memcpy(piece, word, 16);
        for (long i = 0; i < kPiece; i++)
            if (j0 + i >= 0 && j0 + i < row_bytes) out[j0 + i] = piece[i];
    }
}
#endif

}  // namespace kbe_shutter
