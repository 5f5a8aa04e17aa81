// kbe_overlay.hip -- kbe_overlay_u8: an RGBA picture composited onto frames that lie in HBM, in place -- a watermark, a caption --, for
// overlay.py (include/kbe_overlay.h).  The arithmetic is kbe_overlay_block.h's first_pixel() and over_piece(), as they are, and kbe_rows.h's realign(); this file spreads the work over the
// chip (the store of a piece is kbe_rows.h's rule in lines of this kernel's own: see there).  A streaming read-modify-write in the shape of k_transition (kbe_transition.hip): per pixel of the
// clipped rectangle it reads 3 frame bytes and 4 overlay bytes and writes 3, and nothing is read twice.
//
// Only the clipped rectangle is traversed.  A row of it is a byte stream inside a frame's row.  One lane takes one ALIGNED 16-byte piece of
// it; a wave takes kSpan = 1024 bytes of one row, counted from the address of the row's first byte rounded down to 16, and the four waves of
// a workgroup take four rows.  A piece's bytes lie in six pixels: the lane loads the seven aligned dwords that hold the six overlay pixels --
// the first four as one 16-byte piece at a dword's alignment, the rest as one of 12; at a row's two ends dword by dword, and only the
// dwords that hold a byte of a pixel of the rectangle -- and its own 16 frame bytes (at a row's two ends only the dwords that hold a byte of
// the row), all loads in flight together.  A piece that lies inside the row is stored as 16 bytes; the pieces at a row's two ends as
// dwords and single bytes: nothing outside the rectangle is written, and no two lanes write the same byte.  A piece whose six pixels
// all have e = 0 is not stored.
//
// The pointers and every frame's rectangle and opacity travel as kernel arguments: a launch carries kFramesPerLaunch = 12 frames (the
// grid's z), each with a rectangle of its own; the grid is sized by the largest of them.  Every loop has a static bound; no workgroup waits
// for another; no LDS, no scratch.
#include "kbe_overlay.h"
#include "kbe_overlay_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace kov = kbe_overlay;

namespace {

constexpr int kFramesPerLaunch = KBE_OVERLAY_FRAMES_PER_LAUNCH;
constexpr int kRows = 4;                                    // one wave per row
constexpr int kLanes = 64;
constexpr int kSpan = kLanes * kov::kPiece;                 // 1024: the bytes of a row that one workgroup takes
static_assert(kRows * kLanes == kBlock && kSpan == 1024 && kFramesPerLaunch == kbe_rows::kFramesPerLaunch, "the kernel's layout");

using kbe_rows::Dwords3;
using kbe_rows::Dwords4;

struct OverlayArgs {
    uint8_t* frame[kFramesPerLaunch];                       // the first byte of the rectangle in the frame ...
    const uint8_t* overlay[kFramesPerLaunch];               // ... and the overlay pixel that meets it
    uint32_t pixels[kFramesPerLaunch], rows[kFramesPerLaunch], opacity[kFramesPerLaunch];      // the rectangle's size
    uint32_t stride, overlay_stride;
};

__global__ __launch_bounds__(kBlock) void k_overlay(const OverlayArgs a)
{
    const uint32_t lane = threadIdx.x & (kLanes - 1), y = blockIdx.y * kRows + threadIdx.x / kLanes, f = blockIdx.z;
    if (y >= a.rows[f]) return;
    uint8_t* const row = a.frame[f] + (size_t) y * a.stride;
    const int32_t pixels = (int32_t) a.pixels[f];
    const uint32_t lead = (uint32_t) ((uintptr_t) row & 15u), end = lead + 3u * (uint32_t) pixels;      // the row's bytes are [lead, end) of its pieces
    const uint32_t at = blockIdx.x * kSpan + kov::kPiece * lane;                                      // this lane takes the piece [at, at + 16)
    if (at >= end) return;
    const long j0 = (long) at - (long) lead;                                                          // the piece's first byte, as a byte of the row
    const uint32_t lo = at < lead ? lead - at : 0u, hi = end - at < 16u ? end - at : 16u;
    int32_t x0;
    uint32_t r;
    kov::first_pixel(j0, &x0, &r);

    // the overlay's six pixels: (before the row where x0 < 0: not read)
    const uint8_t* const first = a.overlay[f] + (size_t) y * a.overlay_stride + 4l * x0;
    const uint32_t b = (uint32_t) ((uintptr_t) first & 3u);
    const uint32_t* const dwords = reinterpret_cast<const uint32_t*>(first - b);
    uint32_t x[7], c[4];
    if (kov::all_overlay_dwords_hold_a_byte(x0, pixels)) {
        const Dwords4 four = *reinterpret_cast<const Dwords4*>(dwords);
        const Dwords3 three = *reinterpret_cast<const Dwords3*>(dwords + 4);
        x[0] = four.x, x[1] = four.y, x[2] = four.z, x[3] = four.w, x[4] = three.x, x[5] = three.y, x[6] = three.z;
    } else {
        for (int m = 0; m < 7; m++) x[m] = kov::overlay_dword_holds_a_byte(x0, b, m, pixels) ? dwords[m] : 0u;
    }
    // the frame's 16 bytes
    uint8_t* const p = row - lead + at;                                                               // 16-byte aligned
    const bool whole = lo == 0u && hi == 16u;
    if (whole) {
        const uint4 mine = *reinterpret_cast<const uint4*>(p);
        c[0] = mine.x, c[1] = mine.y, c[2] = mine.z, c[3] = mine.w;
    } else {
        for (uint32_t d = 0; d < 4u; d++) c[d] = kov::frame_dword_holds_a_byte(d, lo, hi) ? reinterpret_cast<const uint32_t*>(p)[d] : 0u;
    }

    uint32_t pixel[6], word[4];
    kov::realign(x, b, pixel);
    if (kov::over_piece(pixel, a.opacity[f], r, c, word) == 0u) return;

    // (this kernel's own copy of kbe_rows.h's store_piece: through the shared one it measured 0.15 % slower than with these lines)
    if (whole) *reinterpret_cast<uint4*>(p) = make_uint4(word[0], word[1], word[2], word[3]);
    else {
        for (uint32_t d = 0; d < 4u; d++) {
            if (lo <= 4u * d && 4u * d + 4u <= hi) reinterpret_cast<uint32_t*>(p)[d] = word[d];
            else
                for (uint32_t k = 4u * d; k < 4u * d + 4u; k++)
                    if (lo <= k && k < hi) p[k] = (uint8_t) (word[d] >> (8u * (k & 3u)));
        }
    }
}

}  // namespace

extern "C" {

KBE_OVERLAY_API int kbe_overlay_abi_version(void)
{
    return KBE_OVERLAY_ABI_VERSION;
}

KBE_OVERLAY_API int kbe_overlay_u8(uint8_t* const* frames_u8, int n, int W, int H, int stride_bytes, const uint8_t* overlay_rgba, int w, int h,
                                   int overlay_stride_bytes, const int32_t* x, const int32_t* y, const int32_t* opacity, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!overlay_rgba) what = "null overlay_rgba";
    else if (!x) what = "null x";
    else if (!y) what = "null y";
    else if (!opacity) what = "null opacity";
    else if (n < 1) what = "n < 1";
    else if (!(W >= 1 && W <= kov::kMaxSide && H >= 1 && H <= kov::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (!(w >= 1 && w <= kov::kMaxSide && h >= 1 && h <= kov::kMaxSide)) what = "w or h outside 1..65535";
    else if (overlay_stride_bytes < 4 * w) what = "overlay_stride_bytes < 4 w";
    for (int i = 0; !what && i < n; i++) {
        if (!frames_u8[i]) what = "null element of frames_u8";
        else if (!(x[i] >= -kov::kMaxSide && x[i] <= kov::kMaxSide)) what = "an element of x outside -65535..65535";
        else if (!(y[i] >= -kov::kMaxSide && y[i] <= kov::kMaxSide)) what = "an element of y outside -65535..65535";
        else if (!(opacity[i] >= 0 && opacity[i] <= kov::kMaxOpacity)) what = "an element of opacity outside 0..256";
    }
    // a lane reads and writes its frame's bytes and reads the overlay's: a frame may share no byte with another frame of the call, nor with the overlay
    if (!what) {
        const uintptr_t frame_bytes = frame_extent(H, stride_bytes, 3u * (uintptr_t) W);
        if (any_overlap(frames_u8, n, frame_bytes, &overlay_rgba, 1, frame_extent(h, overlay_stride_bytes, 4u * (uintptr_t) w))) what = "an element of frames_u8 overlaps the overlay";
        else if (any_two_overlap(frames_u8, n, frame_bytes)) what = "an element of frames_u8 overlaps another frame";
    }
    if (what) return refuse("kbe_overlay_u8", what);

    OverlayArgs a;
    a.stride = (uint32_t) stride_bytes;
    a.overlay_stride = (uint32_t) overlay_stride_bytes;
    int held = 0;
    uint32_t most_pixels = 0u, most_rows = 0u;
    const auto launch = [&]() {
        for (int i = held; i < kFramesPerLaunch; i++) a.frame[i] = nullptr, a.overlay[i] = nullptr, a.pixels[i] = a.rows[i] = a.opacity[i] = 0u;
        // (a row's pieces begin up to 15 bytes before the row does)
        const dim3 grid(blocks_for((size_t) 3u * most_pixels + 15u, kSpan), blocks_for((size_t) most_rows, kRows), (unsigned) held);
        hipLaunchKernelGGL(k_overlay, grid, dim3(kBlock), 0, (hipStream_t) stream, a);
        held = 0, most_pixels = most_rows = 0u;
    };
    for (int i = 0; i < n; i++) {
        // the clipped rectangle: the frame's columns [x0, x1) and rows [y0, y1)
        const int x0 = x[i] > 0 ? x[i] : 0, x1 = x[i] + w < W ? x[i] + w : W, y0 = y[i] > 0 ? y[i] : 0, y1 = y[i] + h < H ? y[i] + h : H;
        if (opacity[i] == 0 || x1 <= x0 || y1 <= y0) continue;                   // in no launch
        a.frame[held] = frames_u8[i] + (size_t) y0 * (size_t) stride_bytes + 3u * (size_t) x0;
        a.overlay[held] = overlay_rgba + (size_t) (y0 - y[i]) * (size_t) overlay_stride_bytes + 4u * (size_t) (x0 - x[i]);
        a.pixels[held] = (uint32_t) (x1 - x0), a.rows[held] = (uint32_t) (y1 - y0), a.opacity[held] = (uint32_t) opacity[i];
        most_pixels = a.pixels[held] > most_pixels ? a.pixels[held] : most_pixels;
        most_rows = a.rows[held] > most_rows ? a.rows[held] : most_rows;
        if (++held == kFramesPerLaunch) launch();
    }
    if (held) launch();
    return launched("kbe_overlay_u8");
}

}  // extern "C"
