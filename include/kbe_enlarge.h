/*
 * kbe_enlarge.h -- C ABI of the crop + exact bicubic enlargement of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_enlarge.hip; all of its
 * arithmetic is defined in csrc/kbe_enlarge_block.h, on top of csrc/kbe_crop_area_block.h).  A header of its own beside kbe.h and the other
 * headers here, with a version of its own: their entries and ABI numbers do not change with it.  Errors are reported as by kbe.h's entries:
 * KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through kbe_last_error().  Bound in Python by ken-burns-effect_amd/enlarge.py;
 * common.render_frames(out_size=..., enlarge=True) is its user.
 *
 * A raw W x H frame, a centred crop crop_w x crop_h of it and a target w x h, crop_w <= w <= 16384 and crop_h <= h <= 16384: the entry only
 * enlarges.  The crop is the patch cv2.getRectSubPix takes from the frame's centre, exactly as include/kbe_crop_area.h describes it: bytes.
 * The patch is resampled in ONE step by a separable Catmull-Rom bicubic (a = -1/2) on half-pixel centres, the border pixel repeated: per
 * axis, output x of n_out from n_in lies at ((2 x + 1) n_in - n_out) / (2 n_out) = i + r / D of the patch, its four taps are i - 1 .. i + 2,
 * and their weights are rounded to 14-bit integers that add up to 16384 (three by a floor, the second by difference).  A pass is
 * clamp((sum c_k v_k + 8192) >> 14, 0, 255); the pass along the rows gives bytes, the pass down the columns reads those.  Three roundings:
 * the patch, the rows, the columns.  w == crop_w and h == crop_h give the patch itself.  Integers throughout; channels are not swapped.
 * The bytes are defined by csrc/kbe_enlarge_block.h executed serially on a CPU (tests/enlarge_check.cpp).
 */
#ifndef KBE_ENLARGE_H
#define KBE_ENLARGE_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_ENLARGE_API __attribute__((visibility("default")))
#else
#define KBE_ENLARGE_API
#endif

#define KBE_ENLARGE_ABI_VERSION 1

KBE_ENLARGE_API int kbe_enlarge_abi_version(void);

/* The frames of the encoders' common contract (kbe_gif_encode), cropped and enlarged:
 *   frames_u8: HOST array of n_frames DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535;
 *              any n_frames >= 1 -- the entry cuts them into launches of at most 12 frames;
 *   crop_w, crop_h: the centred crop, 1 <= crop_w <= W, 1 <= crop_h <= H;
 *   out_u8:    HOST array of n_frames DEVICE pointers to [h][out_stride_bytes] rows of 3-byte pixels, out_stride_bytes >= 3 w;
 *              crop_w <= w <= 16384, crop_h <= h <= 16384.  The bytes of an output row beyond 3 w are not written.  No alignment is asked
 *              of any pointer or stride.  An output must not overlap a source.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_ENLARGE_API int kbe_enlarge_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int crop_w, int crop_h,
                                   uint8_t* const* out_u8, int w, int h, int out_stride_bytes, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_ENLARGE_H */
