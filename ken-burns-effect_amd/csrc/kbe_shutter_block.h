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
//     x[0]: w[k] = the dword at byte 4 k + b of x (kbe_rows.h's realign: a funnel shift by bytes).
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

#include "kbe_rows.h"

namespace kbe_shutter {

using kbe_rows::kMaxSide;
using kbe_rows::kPiece;                       // bytes: what one lane of the kernel loads from a source, and stores
using kbe_rows::realign;

constexpr int kMaxSamples = 32;
constexpr int kDwords = kPiece / 4;           // of a piece: a source's lie in kDwords + 1 aligned ones

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

#if !defined(__HIPCC__)
// One output row on a CPU, serially, the way the kernel takes it: pieces of 16 bytes at the OUTPUT row's alignment (`lead` = its address
// modulo 16, given by the caller so that a test can walk through all sixteen), every source realigned by its own address modulo 4
// (row_class[s]: the address of the source row's first byte, any number congruent to it modulo 4).  The walk over the pieces, the aligned
// dwords of a row and the store of a piece are kbe_rows.h's: nothing outside a row is read or written.
inline void mean_row(const uint8_t* const* rows, const uint32_t* row_class, uint32_t S, long row_bytes, uint32_t lead, uint8_t* out)
{
    const uint32_t M = magic(S);
    kbe_rows::for_each_piece(row_bytes, lead, [&](uint32_t at) {
        const long j0 = (long) at - (long) lead;
        Acc acc;
        clear(acc);
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t b = (uint32_t) (((long) row_class[s] + j0) & 3);
            uint32_t x[kDwords + 1], w[kDwords];
            kbe_rows::aligned_dwords<kDwords>(rows[s], j0, b, row_bytes, x);
            realign(x, b, w);
            add(acc, w);
        }
        uint32_t word[4];
        finish(acc, S, M, word);
        kbe_rows::store_piece(out, lead, lead + (uint32_t) row_bytes, at, word);
    });
}
#endif

}  // namespace kbe_shutter
