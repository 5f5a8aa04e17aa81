/*
 * kbe_grade.h -- C ABI of the colour grade of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_grade.hip; all of its arithmetic is defined in
 * csrc/kbe_grade_block.h).  A header of its own beside kbe.h and the other frame filters' headers, with a version of its own: their entries
 * and ABI numbers do not change with it.  Errors are reported as by kbe.h's entries: KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through
 * kbe_last_error().  Bound in Python by ken-burns-effect_amd/grade.py; its users are --lut, --grade and --look.
 *
 * A 3D lookup table with tetrahedral interpolation is applied to frames that lie in HBM, in place.  No floating point.  The table has N
 * nodes per axis, N^3 dwords: entry (i2 * N + i1) * N + i0 is the node at frame byte 0 = i0, byte 1 = i1, byte 2 = i2; its bytes 0..2 are the
 * output's bytes 0..2, byte 3 is ignored.  For a byte v: p = v (N - 1), i = p / 255, f = p - 255 i (v = 255: i = N - 2, f = 255).  With the
 * fractions ordered f_a >= f_b >= f_c: V0 = the cell's base node, V1 = V0 + e_a, V2 = V1 + e_b, V3 = the far corner, and per byte
 *     g   = (V0 (255 - f_a) + V1 (f_a - f_b) + V2 (f_b - f_c) + V3 f_c + 127) / 255       integer division
 *     out = (c (256 - s) + g s + 128) >> 8                                                 the frame's strength s in 0..256
 * A tie between fractions gives the node it decides the weight 0.  The bytes are defined by csrc/kbe_grade_block.h executed serially on a
 * CPU (tests/grade_check.cpp).
 */
#ifndef KBE_GRADE_H
#define KBE_GRADE_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_GRADE_API __attribute__((visibility("default")))
#else
#define KBE_GRADE_API
#endif

#define KBE_GRADE_ABI_VERSION 1
#define KBE_GRADE_FRAMES_PER_LAUNCH 12          /* the entry cuts a call's frames into launches of this many */

KBE_GRADE_API int kbe_grade_abi_version(void);

/*   frames_u8:    HOST array of n >= 1 DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535.
 *                 The frames are read and written in place.  No alignment is asked of a frame pointer or of the stride;
 *   lut:          DEVICE pointer to the table's N^3 dwords, 2 <= N <= 33, 4-byte aligned.  The kernel knows nothing of R, G or B: the
 *                 caller puts the table's axes and bytes into the frames' channel order.  One table serves all n frames;
 *   strength:     HOST array of n values in 0..256: 256 gives the table's colour, 0 leaves the frame as it is.
 * Row padding beyond 3 W is neither read for effect nor written.  A frame whose strength is 0 is in no launch; the others are cut into
 * launches of KBE_GRADE_FRAMES_PER_LAUNCH, their pointer tables travelling as kernel arguments.  Two frames of a call whose byte ranges
 * intersect (the same pointer twice counts) and a frame that intersects the table's bytes are refused.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_GRADE_API int kbe_grade_u8(uint8_t* const* frames_u8, int n, int W, int H, int stride_bytes,
                               const uint32_t* lut, int N, const int32_t* strength, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_GRADE_H */
