/*
 * kbe_gif.h -- C ABI of the device-side animated-GIF encoder of libkbe_hip.so (ken-burns-effect_amd/csrc/kbe_gif.hip; the stream and
 * all of its arithmetic are defined in csrc/kbe_gif_block.h).  A header of its own beside kbe.h, with a version of its own: kbe.h's
 * entries and ABI number do not change with it.  Errors are reported as by kbe.h's entries: KBE_OK / KBE_E_INVALID / KBE_E_LAUNCH, the
 * text through kbe_last_error().  Bound in Python by ken-burns-effect_amd/gif.py, which also assembles the file.
 *
 * The file (gif.py: assemble): GIF89a, logical screen descriptor, ONE global colour table of 256 entries, the NETSCAPE2.0 loop extension,
 * the frames' units back to back, 3B.  A UNIT is what kbe_gif_encode writes per frame: graphic control extension (no transparency, no
 * disposal, delay_cs), image descriptor (full frame, no local table, no interlace), minimum code size 08, the LZW data, 00.  A unit holds
 * no field that depends on its place: the same bytes may appear in a file twice (a video played forth and back).
 *
 * Pixel -> index, integer arithmetic: channels swapped under KBE_GIF_BGR; an ordered dither of amplitude `dither` (0: none; at most 64):
 * v + (bayer8(x & 7, y & 7) * dither >> 6) - (dither >> 1) per channel, clamped to 0..255; the RGB555 cell r5 << 10 | g5 << 5 | b5;
 * index = lut[cell].
 *
 * LZW: the indices in raster order, in independent SEGMENTS of 3838 pixels (the last one short), each coded with a fresh dictionary
 * (Clear 256, EOI 257, first free code 258, 9 to 12 bits by GIF's rule; the 4096 entries cannot fill).  The first segment starts with a
 * Clear; every segment but the last ends with a Clear at the current width and up to 7 Clears of 9 bits that restore the byte boundary; the
 * last ends with EOI.  Every segment's bytes lie in data sub-blocks of its own.  The unit is defined byte for byte by csrc/kbe_gif_block.h
 * executed serially on a CPU (tests/gif_check.cpp).
 */
#ifndef KBE_GIF_H
#define KBE_GIF_H

#include <stddef.h>
#include <stdint.h>

#include "kbe.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KBE_GIF_API __attribute__((visibility("default")))
#else
#define KBE_GIF_API
#endif

#define KBE_GIF_ABI_VERSION 1
#define KBE_GIF_BGR 1

KBE_GIF_API int kbe_gif_abi_version(void);

/* bytes that hold ANY W x H frame's unit -- the true worst case: every code covers one pixel (a sequence of indices in which no adjacent
 * pair repeats inside a segment reaches it exactly).  0 for a size the encoder refuses: W or H outside 1..65535, or a unit that would not
 * stay below 2^31 bytes. */
KBE_GIF_API size_t kbe_gif_bound(int W, int H);
/* the scratch of kbe_gif_encode: 12 bytes per segment of at most 12 frames, and 8 per 256 of them; 0 for a refused size or n_frames < 1 */
KBE_GIF_API size_t kbe_gif_scratch_bytes(int W, int H, int n_frames);

/* The encoders' common contract of kbe.h (kbe_mjpeg_encode, kbe_png_encode), word for word, with the unit above:
 *   frames_u8: HOST array of n_frames DEVICE pointers to [H][stride_bytes] rows of 3-byte pixels (R, G, B; B, G, R with KBE_GIF_BGR),
 *              stride_bytes >= 3 W; W, H <= 65535; any n_frames >= 1 -- the entry cuts them into launches of at most 12 frames;
 *   dither:    the ordered dither's amplitude, 0..64;  delay_cs: a frame's delay in centiseconds, 0..65535;
 *   lut:       DEVICE, 32768 bytes: the palette index of every RGB555 cell (kbe_gif_lut);
 *   out, cap:  frame i's unit is out[offsets[i] .. offsets[i + 1]), the units back to back; NO byte at or beyond cap is written (out may
 *              be NULL when cap is 0);
 *   offsets:   DEVICE [n_frames + 1], 8-byte aligned: the TRUE sizes, whether they fit or not;
 *   status:    DEVICE int: 1 if the units need more than cap bytes (run again with a buffer of offsets[n_frames] bytes), else 0;
 *   scratch:   kbe_gif_scratch_bytes(W, H, n_frames) bytes, 8-byte aligned, contents irrelevant; it grows neither past one launch's
 *              frames nor with the output.
 * Every argument is validated before anything is enqueued (KBE_E_INVALID, kbe_last_error names the entry and the argument); nothing is
 * allocated; all launches are asynchronous on `stream`. */
KBE_GIF_API int kbe_gif_encode(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int flags, int dither, int delay_cs,
                               const uint8_t* lut, void* scratch, uint8_t* out, size_t cap, uint64_t* offsets, int* status, kbe_stream_t stream);

/* hist[cell] += the number of pixels of the n_frames frames (the same frames_u8, W, H, stride_bytes and KBE_GIF_BGR as above) in each RGB555
 * cell; no dither.  hist: DEVICE uint32 [32768] that the caller has zeroed; several calls accumulate. */
KBE_GIF_API int kbe_gif_histogram(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int flags, uint32_t* hist, kbe_stream_t stream);

/* lut[cell] = the index of the palette entry nearest to the cell's centre colour ((v5 << 3) | (v5 >> 2) per channel): squared Euclidean
 * distance in RGB, ties to the lowest index.  palette: DEVICE, 3 * n_colors bytes (R, G, B), 1 <= n_colors <= 256; lut: DEVICE, 32768 bytes. */
KBE_GIF_API int kbe_gif_lut(const uint8_t* palette, int n_colors, uint8_t* lut, kbe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KBE_GIF_H */
