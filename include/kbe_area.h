/*
 * kbe_area.h -- C ABI of the exact area-average reduction of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_area.hip; all of its arithmetic
 * is defined in csrc/kbe_area_block.h).  A header of its own beside kbe.h and kbe_gif.h, with a version of its own: their entries and ABI
 * numbers do not change with it.  Errors are reported as by kbe.h's entries: KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through
 * kbe_last_error().  Bound in Python by ken-burns-effect_amd/area.py; gif.write_gif(size=...) is its user.
 *
 * W x H frames become w x h frames, w <= W and h <= H: the entry only reduces.  Integer arithmetic, per axis (N source cells, n target
 * cells) on an axis of N n units where source cell s covers [s n, (s + 1) n) and target cell o covers [o N, (o + 1) N); weight(o, s) is the
 * length of their overlap.  Per channel S = sum of weight_y * weight_x * v over the source, out = (2 S + W H) / (2 W H) in integer division:
 * the area-weighted mean, rounded half up.  w == W and h == H copies.  Channels are not swapped.  The bytes are defined by
 * csrc/kbe_area_block.h executed serially on a CPU (tests/area_check.cpp).
 */
#ifndef KBE_AREA_H
#define KBE_AREA_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_AREA_API __attribute__((visibility("default")))
#else
#define KBE_AREA_API
#endif

#define KBE_AREA_ABI_VERSION 1

KBE_AREA_API int kbe_area_abi_version(void);

/* The frames of the encoders' common contract (kbe_gif_encode), reduced:
 *   frames_u8: HOST array of n_frames DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535;
 *              any n_frames >= 1 -- the entry cuts them into launches of at most 12 frames;
 *   out_u8:    HOST array of n_frames DEVICE pointers to [h][out_stride_bytes] rows of 3-byte pixels, out_stride_bytes >= 3 w;
 *              1 <= w <= W, 1 <= h <= H.  The bytes of an output row beyond 3 w are not written.  No alignment is asked of any pointer or
 *              stride.  An output must not overlap a source.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_AREA_API int kbe_area_reduce_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes,
                                    uint8_t* const* out_u8, int w, int h, int out_stride_bytes, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_AREA_H */
