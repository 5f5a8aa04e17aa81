// kbe_enlarge.hip -- kbe_enlarge_u8: raw frames that lie in HBM, their centred crop enlarged by the exact integer bicubic, for enlarge.py
// (include/kbe_enlarge.h).  The arithmetic is kbe_enlarge_block.h's taps() and pass() on kbe_crop_area_block.h's patch, as they are; this
// file spreads the work over the chip.
//
// One workgroup takes a TILE of kTileX x kTileY target pixels of one frame (the frame is the grid's z).  The entry only enlarges, so the
// tile's taps lie in a SPAN of at most kSpanPx x kSpanRows patch pixels, and under it lies its span of the RAW frame: one row and one
// pixel more (the second taps of a half-pixel start).  Per tile
//   (0) the taps of the tile's columns and rows are made ONCE, a lane per column and a lane per row (each coefficient costs a 64-bit
//       division), into LDS, the taps relative to the span;
//   (1) the raw rows are fetched as aligned dwords; a row's first pixel lies 0..3 bytes into its LDS row;
//   (2) the span's patch bytes are made once in LDS from the staged raw rows.  A crop that starts on whole pixels on both axes IS the
//       raw rectangle: the step is skipped and (3) reads the staged raw rows.  The test is uniform over the launch;
//   (3) the pass along the rows: every row of the span, at the tile's columns, into a plane of bytes in LDS;
//   (4) the pass down the columns out of that plane, into the tile's bytes in LDS at the output rows' own alignment modulo 16;
//   (5) the rows are stored as 16-byte pieces, with dwords and single bytes only where a row's ends do not fill a piece; nothing outside a
//       row's 3 w bytes is written.
// The row fetch's arithmetic in (1), the tile's row in LDS in (4) and its store in (5) are kbe_rows.h's, which the other tile kernels run too.
// A tile is 16 rows high so that (3), which runs once per row of the span, is shared by many output rows.  Every loop has a static bound;
// no workgroup waits for another; there are no tables in device memory.
#include "kbe_enlarge.h"
#include "kbe_enlarge_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace kca = kbe_crop_area;
namespace ken = kbe_enlarge;

namespace {

using kbe_rows::kFramesPerLaunch;
constexpr int kTileX = 64, kTileY = 16;
// n target indices in a row lie within ceil((n - 1) n_in / n_out) <= n - 1 values of i, and the taps are i - 1 .. i + 2
constexpr int kSpanPx = kTileX + 3, kSpanRows = kTileY + 3;
constexpr int kRawPx = kSpanPx + 1, kRawRows = kSpanRows + 1;
constexpr int kRawDwords = (3 + 3 * kRawPx + 3) / 4;        // 52: 0..3 bytes of misalignment and 204 of pixels
constexpr int kPatchPitch = (3 * kSpanPx + 3) / 4 * 4;      // 204 bytes
constexpr int kPlanePitch = 3 * kTileX;                     // 192 bytes: a row of the span at the tile's columns
constexpr int kOutPitch = 3 * kTileX + 16;                  // a tile's row of 192 bytes, 0..15 bytes into its LDS row
constexpr int kPieces = kOutPitch / 16;                     // 13
constexpr int kRawWords = kRawRows * kRawDwords, kPatchWords = (kSpanRows * kPatchPitch / 4 + 3) / 4 * 4, kPlaneWords = kSpanRows * kPlanePitch / 4, kOutWords = kTileY * kOutPitch / 4;
constexpr int kStageTrips = (kRawWords + kBlock - 1) / kBlock, kPlaneTrips = (kSpanRows * kPlanePitch + kBlock - 1) / kBlock, kOutTrips = kTileY * kPlanePitch / kBlock;
static_assert(kTileX + kTileY <= kBlock && 3 * kSpanPx <= kBlock && kTileY * 16 == kBlock && kPieces <= 16 && kOutPitch % 16 == 0 && (kTileY * kPlanePitch) % kBlock == 0 &&
              (kRawWords + kPatchWords + kPlaneWords) % 4 == 0, "the kernel's layout");

struct EnlargeArgs {
    const uint8_t* src[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    kca::Crop k;
    uint32_t w, h, stride, out_stride;
};

__global__ __launch_bounds__(kBlock) void k_enlarge(const EnlargeArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_words[kRawWords + kPatchWords + kPlaneWords + kOutWords];
    __shared__ ken::Taps s_taps[kTileX + kTileY];            // the tile's columns, then its rows
    uint8_t* const s_raw = reinterpret_cast<uint8_t*>(s_words);
    uint8_t* const s_patch = reinterpret_cast<uint8_t*>(s_words + kRawWords);
    uint8_t* const s_plane = reinterpret_cast<uint8_t*>(s_words + kRawWords + kPatchWords);
    uint8_t* const s_out = reinterpret_cast<uint8_t*>(s_words + kRawWords + kPatchWords + kPlaneWords);

    const kca::Crop k = a.k;
    const uint32_t tid = threadIdx.x;
    const uint32_t ox0 = blockIdx.x * kTileX, oy0 = blockIdx.y * kTileY;
    const uint32_t nx = a.w - ox0 < (uint32_t) kTileX ? a.w - ox0 : (uint32_t) kTileX, ny = a.h - oy0 < (uint32_t) kTileY ? a.h - oy0 : (uint32_t) kTileY;
    // the tile's span of the patch (the same in every lane): the first tap of its first index to the last tap of its last, clamped
    uint32_t r;
    const uint32_t px0 = ken::clamped(ken::position(k.cw, a.w, ox0, &r) - 1, k.cw), px1 = ken::clamped(ken::position(k.cw, a.w, ox0 + nx - 1u, &r) + 2, k.cw) + 1u;
    const uint32_t py0 = ken::clamped(ken::position(k.ch, a.h, oy0, &r) - 1, k.ch), py1 = ken::clamped(ken::position(k.ch, a.h, oy0 + ny - 1u, &r) + 2, k.ch) + 1u;
    const uint32_t n_px = px1 - px0, n_rows = py1 - py0;                                    // at most kSpanPx, kSpanRows
    // where the span lies in the raw frame: its second taps too, as far as the frame goes
    const uint32_t hx = kca::half(k.W, k.cw) ? 1u : 0u, hy = kca::half(k.H, k.ch) ? 1u : 0u;
    const bool whole = kca::whole(k);
    const uint32_t rx0 = kca::start(k.W, k.cw) + px0, rx1 = rx0 + n_px + hx < k.W ? rx0 + n_px + hx : k.W;            // at most kRawPx pixels
    const uint32_t ry0 = kca::start(k.H, k.ch) + py0, ry1 = ry0 + n_rows + hy < k.H ? ry0 + n_rows + hy : k.H;        // at most kRawRows rows
    const uint8_t* const src = a.src[blockIdx.z];

    // (0)
    if (tid < nx) {
        ken::Taps t = ken::taps(k.cw, a.w, ox0 + tid);
        for (int j = 0; j < 4; j++) t.t[j] -= px0;
        s_taps[tid] = t;
    } else if (tid >= (uint32_t) kTileX && tid - kTileX < ny) {
        ken::Taps t = ken::taps(k.ch, a.h, oy0 + tid - kTileX);
        for (int j = 0; j < 4; j++) t.t[j] -= py0;
        s_taps[tid] = t;
    }
    // (1) the aligned dwords that hold a byte of pixels rx0 .. rx1 - 1 of raw row ry: every one of them holds a byte of the row
    for (int trip = 0; trip < kStageTrips; trip++) {
        const uint32_t at = tid + (uint32_t) trip * kBlock, row = at / kRawDwords, d = at - row * kRawDwords;
        if (row >= ry1 - ry0) break;
        const kbe_rows::Fetch raw = kbe_rows::fetch_of(src + (size_t) (ry0 + row) * a.stride + 3u * (size_t) rx0, rx1 - rx0);
        if (d < raw.dwords) s_words[at] = raw.base[d];
    }
    __syncthreads();
    // raw row ry, from its pixel rx0 on, starts (its address mod 4) bytes into LDS row ry - ry0
    auto raw_row = [&](uint32_t ry) -> const uint8_t* {
        return s_raw + (ry - ry0) * (4u * kRawDwords) + kbe_rows::shift_of(src + (size_t) ry * a.stride + 3u * (size_t) rx0);
    };
    // (2) the span's patch bytes: byte column b is channel b % 3 of patch pixel px0 + b / 3; a thread owns one and walks down the rows
    if (!whole) {
        const uint32_t b = tid;
        if (b < 3u * n_px) {
            const uint32_t px = b / 3u, c = b - 3u * px;
            const uint32_t o0 = 3u * (kca::tap0(k.W, k.cw, px0 + px) - rx0) + c, o1 = 3u * (kca::tap1(k.W, k.cw, px0 + px) - rx0) + c;
            for (uint32_t pr = 0; pr < (uint32_t) kSpanRows; pr++) {
                if (pr >= n_rows) break;
                const uint8_t* const r0 = raw_row(kca::tap0(k.H, k.ch, py0 + pr));
                const uint8_t* const r1 = raw_row(kca::tap1(k.H, k.ch, py0 + pr));
                s_patch[pr * kPatchPitch + b] = (uint8_t) kca::patch_value(r0[o0], r0[o1], r1[o0], r1[o1]);
            }
        }
        __syncthreads();
    }
    // (3) the pass along the rows: byte b of row pr of the plane is channel b % 3 of column b / 3 of the tile
    for (int trip = 0; trip < kPlaneTrips; trip++) {
        const uint32_t at = tid + (uint32_t) trip * kBlock, pr = at / kPlanePitch, b = at - pr * kPlanePitch, col = b / 3u, c = b - 3u * col;
        if (pr >= n_rows) break;
        if (col >= nx) continue;
        const uint8_t* const row = whole ? raw_row(ry0 + pr) : s_patch + pr * kPatchPitch;
        const ken::Taps& t = s_taps[col];
        s_plane[at] = (uint8_t) ken::pass(t.c, row[3u * t.t[0] + c], row[3u * t.t[1] + c], row[3u * t.t[2] + c], row[3u * t.t[3] + c]);
    }
    __syncthreads();
    // (4) the pass down the columns; row ty of the tile starts (its address mod 16) bytes into its LDS row
    uint8_t* const dst = a.dst[blockIdx.z];
    for (int trip = 0; trip < kOutTrips; trip++) {
        const uint32_t at = tid + (uint32_t) trip * kBlock, ty = at / kPlanePitch, b = at - ty * kPlanePitch;
        if (ty >= ny) break;
        if (b >= 3u * nx) continue;
        const ken::Taps& t = s_taps[kTileX + ty];
        const uint32_t lead = kbe_rows::lead_of(dst + (size_t) (oy0 + ty) * a.out_stride + 3u * (size_t) ox0);
        s_out[ty * kOutPitch + lead + b] = (uint8_t) ken::pass(t.c, s_plane[t.t[0] * kPlanePitch + b], s_plane[t.t[1] * kPlanePitch + b], s_plane[t.t[2] * kPlanePitch + b], s_plane[t.t[3] * kPlanePitch + b]);
    }
    __syncthreads();
    // (5) sixteen lanes per row of the tile, lane `piece` of them takes the bytes [16 piece, 16 piece + 16) of the LDS row
    const uint32_t ty = tid / 16u, at = 16u * (tid & 15u);
    if (ty < ny) kbe_rows::store_tile_row(s_out + ty * kOutPitch, dst + (size_t) (oy0 + ty) * a.out_stride + 3u * (size_t) ox0, nx, at);
}

}  // namespace

extern "C" {

KBE_ENLARGE_API int kbe_enlarge_abi_version(void)
{
    return KBE_ENLARGE_ABI_VERSION;
}

KBE_ENLARGE_API int kbe_enlarge_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int crop_w, int crop_h, uint8_t* const* out_u8, int w, int h,
                                   int out_stride_bytes, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!out_u8) what = "null out_u8";
    else if (n_frames < 1) what = "n_frames < 1";
    else if (!(W >= 1 && W <= kbe_rows::kMaxSide && H >= 1 && H <= kbe_rows::kMaxSide)) what = "W or H outside 1..65535";
    else if (!(crop_w >= 1 && crop_w <= W)) what = "crop_w outside 1..W";
    else if (!(crop_h >= 1 && crop_h <= H)) what = "crop_h outside 1..H";
    else if (!(w >= crop_w && w <= ken::kMaxOut)) what = "w outside crop_w..16384: the entry only enlarges";
    else if (!(h >= crop_h && h <= ken::kMaxOut)) what = "h outside crop_h..16384: the entry only enlarges";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (out_stride_bytes < 3 * w) what = "out_stride_bytes < 3 w";
    for (int i = 0; !what && i < n_frames; i++)
        if (!frames_u8[i] || !out_u8[i]) what = frames_u8[i] ? "null element of out_u8" : "null element of frames_u8";
    if (what) return refuse("kbe_enlarge_u8", what);

    EnlargeArgs a;
    a.k = kca::Crop{(uint32_t) W, (uint32_t) H, (uint32_t) crop_w, (uint32_t) crop_h};
    a.w = (uint32_t) w;
    a.h = (uint32_t) h;
    a.stride = (uint32_t) stride_bytes;
    a.out_stride = (uint32_t) out_stride_bytes;
    const dim3 tiles(blocks_for((size_t) w, kTileX), blocks_for((size_t) h, kTileY));
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = launch_frames(n_frames, f0, kFramesPerLaunch);
        fill_slots(a.src, frames_u8, f0, nf);
        fill_slots(a.dst, out_u8, f0, nf);
        hipLaunchKernelGGL(k_enlarge, dim3(tiles.x, tiles.y, (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_enlarge_u8");
}

}  // extern "C"
