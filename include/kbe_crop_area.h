/*
 * kbe_crop_area.h -- C ABI of the crop + exact area-average reduction of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_crop_area.hip; all
 * of its arithmetic is defined in csrc/kbe_crop_area_block.h, on top of csrc/kbe_area_block.h).  A header of its own beside kbe.h, kbe_gif.h
 * and kbe_area.h, with a version of its own: their entries and ABI numbers do not change with it.  Errors are reported as by kbe.h's
 * entries: KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through kbe_last_error().  Bound in Python by ken-burns-effect_amd/crop_area.py;
 * common.render_frames(out_size=...) is its user.
 *
 * A raw W x H frame, a centred crop crop_w x crop_h of it and a target w x h, w <= crop_w and h <= crop_h: the entry only reduces.  The
 * crop is the patch cv2.getRectSubPix takes from the frame's centre (kbe_crop_resize_u8's first step): per axis it starts at
 * N / 2 - (n - 1) / 2, on a whole pixel when N - n is odd and half a pixel further when it is even; a patch pixel is then the raw pixel,
 * (a + b + 1) >> 1 of two raw neighbours, or (a + b + c + d + 2) >> 2 of 2 x 2, a tap beyond the frame repeating the border pixel.  The
 * patch is reduced as include/kbe_area.h reduces a crop_w x crop_h frame to w x h: the area-weighted mean, rounded half up.  Two roundings:
 * the patch to a byte, then the mean.  Channels are not swapped.  The bytes are defined by csrc/kbe_crop_area_block.h executed serially on
 * a CPU (tests/crop_area_check.cpp).
 */
#ifndef KBE_CROP_AREA_H
#define KBE_CROP_AREA_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_CROP_AREA_API __attribute__((visibility("default")))
#else
#define KBE_CROP_AREA_API
#endif

#define KBE_CROP_AREA_ABI_VERSION 1

KBE_CROP_AREA_API int kbe_crop_area_abi_version(void);

/* The frames of the encoders' common contract (kbe_gif_encode), cropped and reduced:
 *   frames_u8: HOST array of n_frames DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535;
 *              any n_frames >= 1 -- the entry cuts them into launches of at most 12 frames;
 *   crop_w, crop_h: the centred crop, 1 <= crop_w <= W, 1 <= crop_h <= H;
 *   out_u8:    HOST array of n_frames DEVICE pointers to [h][out_stride_bytes] rows of 3-byte pixels, out_stride_bytes >= 3 w;
 *              1 <= w <= crop_w, 1 <= h <= crop_h.  The bytes of an output row beyond 3 w are not written.  No alignment is asked of any
 *              pointer or stride.  An output must not overlap a source.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_CROP_AREA_API int kbe_crop_area_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int crop_w, int crop_h,
                                       uint8_t* const* out_u8, int w, int h, int out_stride_bytes, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_CROP_AREA_H */
