/*
 * kbe_transition.h -- C ABI of the transitions of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_transition.hip; all of its arithmetic is defined
 * in csrc/kbe_transition_block.h).  A header of its own beside kbe.h, kbe_gif.h, kbe_area.h, kbe_crop_area.h, kbe_dof.h, kbe_shutter.h and
 * kbe_yuv.h, with a version of its own: their entries and ABI numbers do not change with it.  Errors are reported as by kbe.h's entries:
 * KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the text through kbe_last_error().  Bound in Python by ken-burns-effect_amd/transition.py;
 * transition.join is its user: a slideshow, several clips in one video, the frames at every junction made of a frame of each clip.
 *
 * One output frame is made of two source frames, `from` and `to`, byte by byte.  No floating point.  With
 *     blend(a, b, w) = (a (256 - w) + b w + 128) >> 8        for w in 0..256
 * an output byte is blend(from, to, w); the weight w of the byte's pixel (x, y) comes from the kind, the frame's progress p in 0..256 and,
 * for the wipes, the softness s:
 *     KBE_TRANSITION_DISSOLVE     w = p
 *     KBE_TRANSITION_WIPE_RIGHT   _LEFT, _DOWN, _UP: with (t, L) = (x, W), (W - 1 - x, W), (y, H), (H - 1 - y, H):
 *                                 num = p (L + s) - 256 t;  w = 0 if num <= 0, else min(256, num / s) in integer division: an edge s pixels
 *                                 soft that has crossed the frame when p is 256
 *     KBE_TRANSITION_FADE         through a colour: p <= 128: blend(from, colour byte, 2 p); otherwise blend(colour byte, to, 2 p - 256)
 * p = 0 gives `from` byte for byte and p = 256 gives `to`, for every kind; from == to gives that frame under the dissolve and every wipe.
 * The bytes are defined by csrc/kbe_transition_block.h executed serially on a CPU (tests/transition_check.cpp).
 */
#ifndef KBE_TRANSITION_H
#define KBE_TRANSITION_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_TRANSITION_API __attribute__((visibility("default")))
#else
#define KBE_TRANSITION_API
#endif

#define KBE_TRANSITION_ABI_VERSION 1

#define KBE_TRANSITION_DISSOLVE 0
#define KBE_TRANSITION_WIPE_RIGHT 1
#define KBE_TRANSITION_WIPE_LEFT 2
#define KBE_TRANSITION_WIPE_DOWN 3
#define KBE_TRANSITION_WIPE_UP 4
#define KBE_TRANSITION_FADE 5
#define KBE_TRANSITION_FRAMES_PER_LAUNCH 12     /* the entry cuts a call's frames into launches of this many */

KBE_TRANSITION_API int kbe_transition_abi_version(void);

/* The frames of kbe_shutter_mean_u8's contract, two to one:
 *   from_u8, to_u8: HOST arrays of n DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W; 1 <= W, H <= 65535.
 *              from_u8[i] may equal or overlap to_u8[i] or any other source;
 *   n:         any number >= 1 of output frames.  The pointer tables travel as kernel arguments: the entry cuts the frames into launches
 *              of KBE_TRANSITION_FRAMES_PER_LAUNCH;
 *   kind:      one of the six above;
 *   progress:  HOST array of n values p in 0..256, one per frame;
 *   softness:  s in 1..65535, pixels along the wipe's axis; read by the wipes only, validated always;
 *   colour:    read by the fade only: byte k = 0, 1, 2 of a pixel meets (colour >> 8 k) & 255.  Bits 24..31 set: refused;
 *   out_u8:    HOST array of n DEVICE pointers to [H][out_stride_bytes] rows of 3-byte pixels, out_stride_bytes >= 3 W.  The bytes of an
 *              output row beyond 3 W are not written.  No alignment is asked of any pointer or stride.  The byte range of an output must
 *              not intersect the byte range of any source frame of the call, nor that of another output: both are refused.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_TRANSITION_API int kbe_transition_u8(const uint8_t* const* from_u8, const uint8_t* const* to_u8, int n, int W, int H, int stride_bytes,
                                         int kind, const int32_t* progress, int softness, uint32_t colour,
                                         uint8_t* const* out_u8, int out_stride_bytes, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_TRANSITION_H */
