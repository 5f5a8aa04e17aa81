/*
 * kbe_yuv.h -- C ABI of the 4:2:0 video planes of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_yuv.hip; all of its arithmetic is defined in
 * csrc/kbe_yuv_block.h).  A header of its own beside the library's other headers, with a version of its own: their entries and ABI numbers do
 * not change with it.  Errors are reported as by kbe.h's entries: KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through kbe_last_error().
 * Bound in Python by ken-burns-effect_amd/yuv.py; yuv.write_y4m (Pipeline(y4m=True), kbe.py --y4m) is its user: a clip as the uncompressed
 * YUV4MPEG2 stream that video encoders and players read.
 *
 * A frame of H x W 3-byte pixels becomes planar Y'CbCr 4:2:0, BT.601 at limited range, in integers.  With R, G, B a pixel's bytes (after
 * KBE_YUV_BGR has swapped the first and the third):
 *     Y  = 16 + ((66 R + 129 G + 25 B + 128) >> 8)                          for every pixel, 16..235;
 *     Cb = 128 + floor((-38 Rs - 74 Gs + 112 Bs + 128 n) / (256 n)),
 *     Cr = 128 + floor((112 Rs - 94 Gs - 18 Bs + 128 n) / (256 n))          for every chroma cell, 16..240;
 * there are cw x ch cells, cw = (W + 1) / 2, ch = (H + 1) / 2; cell (cx, cy) covers the pixels x in {2 cx, 2 cx + 1}, y in {2 cy, 2 cy + 1}
 * that exist, n = 1, 2 or 4 of them, and Rs, Gs, Bs are their sums: the chroma site is the cell's centre, which is what C420jpeg says.  The
 * payload of a frame is W H + 2 cw ch contiguous bytes: the Y plane (rows of W), the Cb plane (rows of cw), the Cr plane -- the bytes that
 * follow "FRAME\n" in a C420jpeg y4m stream.  No floating point.  The bytes are defined by csrc/kbe_yuv_block.h executed serially on a CPU
 * (tests/yuv_check.cpp).
 */
#ifndef KBE_YUV_H
#define KBE_YUV_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_YUV_API __attribute__((visibility("default")))
#else
#define KBE_YUV_API
#endif

#define KBE_YUV_ABI_VERSION 1
#define KBE_YUV_BGR 1                   /* flags: a pixel's bytes are B, G, R */
#define KBE_YUV_FRAMES_PER_LAUNCH 12    /* the entry cuts n_frames into launches of this many frames */

KBE_YUV_API int kbe_yuv_abi_version(void);

/* The bytes of one frame's payload: W H + 2 ((W + 1) / 2) ((H + 1) / 2); 0 where W or H is outside 1..65535. */
KBE_YUV_API size_t kbe_yuv420_bytes(int W, int H);

/* The frames of the other frame filters' contract, each converted into a payload:
 *   frames_u8: HOST array of n_frames DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535;
 *   n_frames:  any number >= 1.  The pointer tables travel as kernel arguments: the entry cuts the frames into launches of
 *              KBE_YUV_FRAMES_PER_LAUNCH frames;
 *   out_u8:    HOST array of n_frames DEVICE pointers to kbe_yuv420_bytes(W, H) bytes each.  No byte outside them is written.  No alignment
 *              is asked of any pointer or stride.  The byte range of an output must not intersect the byte range of any source frame of
 *              the call, nor that of another output: both are refused;
 *   flags:     0 or KBE_YUV_BGR; any other bit is refused.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_YUV_API int kbe_yuv420_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, uint8_t* const* out_u8, int flags,
                              kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_YUV_H */
