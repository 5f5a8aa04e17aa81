/*
 * kbe_overlay.h -- C ABI of the overlay of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_overlay.hip; all of its arithmetic is defined in
 * csrc/kbe_overlay_block.h).  A header of its own beside kbe.h, kbe_gif.h, kbe_area.h, kbe_crop_area.h, kbe_dof.h, kbe_shutter.h, kbe_yuv.h and
 * kbe_transition.h, with a version of its own: their entries and ABI numbers do not change with it.  Errors are reported as by kbe.h's
 * entries: KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through kbe_last_error().  Bound in Python by ken-burns-effect_amd/overlay.py;
 * its users are a watermark (--overlay) and captions (--caption).
 *
 * An RGBA picture is composited onto frames that lie in HBM, in place.  No floating point.  For a frame byte c, the overlay byte o of the
 * same channel, the overlay pixel's alpha a (straight, not premultiplied) and the frame's opacity in 0..256:
 *     e   = (a * opacity + 128) >> 8                  0..255
 *     out = (c * (255 - e) + o * e + 127) / 255       integer division: the nearest value (255 is odd: there is no tie)
 * e = 0 gives c, e = 255 gives o, c == o gives c.  The bytes are defined by csrc/kbe_overlay_block.h executed serially on a CPU
 * (tests/overlay_check.cpp).
 */
#ifndef KBE_OVERLAY_H
#define KBE_OVERLAY_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_OVERLAY_API __attribute__((visibility("default")))
#else
#define KBE_OVERLAY_API
#endif

#define KBE_OVERLAY_ABI_VERSION 1
#define KBE_OVERLAY_FRAMES_PER_LAUNCH 12        /* the entry cuts a call's frames into launches of this many */

KBE_OVERLAY_API int kbe_overlay_abi_version(void);

/*   frames_u8:    HOST array of n >= 1 DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535.
 *                 The frames are read and written in place.  No alignment is asked of any pointer or stride;
 *   overlay_rgba: DEVICE pointer to [h][overlay_stride_bytes] rows of 4-byte pixels, overlay_stride_bytes >= 4 w; 1 <= w, h <= 65535.
 *                 Bytes 0..2 of an overlay pixel meet bytes 0..2 of a frame pixel (the caller puts them in the frames' channel order),
 *                 byte 3 is alpha.  One overlay serves all n frames;
 *   x, y:         HOST arrays of n values in -65535..65535: where the overlay's top-left pixel lies in frame i.  What falls outside the
 *                 frame is clipped; an overlay wholly outside leaves the frame as it is;
 *   opacity:      HOST array of n values in 0..256.
 * No byte outside the clipped rectangle is written, not even with its old value; row padding beyond 3 W is neither read for effect nor
 * written.  A frame whose opacity is 0 or whose clipped rectangle is empty is in no launch; the others are cut into launches of
 * KBE_OVERLAY_FRAMES_PER_LAUNCH, their pointer tables travelling as kernel arguments.  Two frames of a call whose byte ranges intersect
 * (the same pointer twice counts) and a frame that intersects the overlay's byte range are refused.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_OVERLAY_API int kbe_overlay_u8(uint8_t* const* frames_u8, int n, int W, int H, int stride_bytes,
                                   const uint8_t* overlay_rgba, int w, int h, int overlay_stride_bytes,
                                   const int32_t* x, const int32_t* y, const int32_t* opacity, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_OVERLAY_H */
