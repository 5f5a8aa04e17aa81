/*
 * kbe_shutter.h -- C ABI of the shutter mean of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_shutter.hip; all of its arithmetic is defined in
 * csrc/kbe_shutter_block.h).  A header of its own beside kbe.h, kbe_gif.h, kbe_area.h, kbe_crop_area.h and kbe_dof.h, with a version of its
 * own: their entries and ABI numbers do not change with it.  Errors are reported as by kbe.h's entries: KBE_OK / KBE_E_INVALID /
 * KBE_E_LAUNCH, the text through kbe_last_error().  Bound in Python by ken-burns-effect_amd/shutter.py; common.render_frames(shutter=...)
 * is its user: motion blur, every frame of a clip the mean of frames rendered at sub-frame cameras while the shutter is open.
 *
 * One output frame is the mean of `samples` source frames, byte by byte: with sum the sum of the S source bytes of a byte position,
 * out = (2 sum + S) / (2 S) in integer division -- the mean, rounded half up.  1 <= S <= 32.  Channels are not looked at: a row is 3 W
 * bytes.  S = 1 copies.  The same source may appear more than once among the S, which weighs it.  No floating point.  The bytes are defined
 * by csrc/kbe_shutter_block.h executed serially on a CPU (tests/shutter_check.cpp).
 */
#ifndef KBE_SHUTTER_H
#define KBE_SHUTTER_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_SHUTTER_API __attribute__((visibility("default")))
#else
#define KBE_SHUTTER_API
#endif

#define KBE_SHUTTER_ABI_VERSION 1

KBE_SHUTTER_API int kbe_shutter_abi_version(void);

/* The frames of kbe_dof_u8's contract, averaged in groups of `samples`:
 *   frames_u8: HOST array of n_out * samples DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels, stride_bytes >= 3 W;
 *              1 <= W, H <= 65535.  The sources of output i are frames_u8[i * samples .. i * samples + samples - 1].  Sources may repeat
 *              and may overlap one another;
 *   n_out:     any number >= 1 of output frames.  The pointer tables travel as kernel arguments: the entry cuts the outputs into launches
 *              of min(12, max(1, 96 / samples)) output frames, so that a launch carries at most 96 source pointers -- 12 outputs up to
 *              samples = 8, 3 at samples = 32;
 *   samples:   1..32;
 *   out_u8:    HOST array of n_out DEVICE pointers to [H][out_stride_bytes] rows of 3-byte pixels, out_stride_bytes >= 3 W.  The bytes of
 *              an output row beyond 3 W are not written.  No alignment is asked of any pointer or stride.  The byte range of an output
 *              must not intersect the byte range of any source frame of the call, nor that of another output: both are refused.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated, there is no scratch; all launches are asynchronous on `stream`. */
KBE_SHUTTER_API int kbe_shutter_mean_u8(const uint8_t* const* frames_u8, int n_out, int samples, int W, int H, int stride_bytes,
                                        uint8_t* const* out_u8, int out_stride_bytes, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_SHUTTER_H */
