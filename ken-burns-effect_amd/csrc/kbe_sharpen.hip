// kbe_sharpen.hip -- kbe_sharpen_u8: frames that lie in HBM, sharpened by the exact integer unsharp mask, for sharpen.py
// (include/kbe_sharpen.h).  The arithmetic is kbe_sharpen_block.h's row_pass(), column_pass() and sharpened(), as they are; this file
// spreads the work over the chip.
//
// One workgroup takes a TILE of kTileX x kTileY pixels of one frame (the frame is the grid's z) and, with R the call's radius,
//   (1) stages the tile's rows and R more above and below -- a row beyond the frame is the border row again -- as aligned dwords: the
//       tile's pixels and up to R more on either side, as far as the frame goes; a row's first pixel lies 0..3 bytes into its dwords;
//   (1b) a tile at the frame's left or right border repeats the border pixel into the halo the frame does not have, so that (2) reads
//       every tap at a fixed distance;
//   (2) the pass along the rows: every staged row at the tile's byte columns, into a plane of 16-bit values;
//   (3) the pass down the columns out of that plane, the difference to the staged byte, the threshold, the gain and the clamp, into the
//       tile's bytes in LDS at the output rows' own alignment modulo 16;
//   (4) the rows are stored as 16-byte pieces, with dwords and single bytes only where a row's ends do not fill a piece; nothing outside
//       a row's 3 W bytes is written.
// The row fetch's arithmetic in (1), the tile's row in LDS in (3) and its store in (4) are kbe_rows.h's, which the other tile kernels run too.
// The tile is 64 x 32: (2) runs once per staged row, 32 + 2 R of them for 32 rows of output -- 2.5 times over at R = 24, where a tile 16
// rows high would take 4 -- and the LDS a workgroup asks for follows R (lds_bytes): 26 784 bytes at R = 1, 29 616 at R = 3, 65 216 at R = 24,
// so that at the radii of everyday sigmas five workgroups share a CU's 160 KiB, and two at R = 24.  The taps travel in the kernel's arguments.  Every loop has
// a static bound; no workgroup waits for another; there are no tables in device memory.
#include "kbe_sharpen.h"
#include "kbe_sharpen_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace ksh = kbe_sharpen;

namespace {

using kbe_rows::kFramesPerLaunch;
constexpr int kTileX = 64, kTileY = 32;
constexpr int kRowBytes = 3 * kTileX;                        // 192: a row of the tile, and of the plane, in values
constexpr int kOutPitch = kRowBytes + 16;                    // a tile's row of 192 bytes, 0..15 bytes into its LDS row
constexpr int kPieces = kOutPitch / 16;                      // 13
constexpr int kOutWords = kTileY * kOutPitch / 4;

// A staged row: up to 3 bytes so that the frame's first dword lands on a dword behind a left halo, 0..3 bytes of misalignment, the
// 3 (kTileX + 2 R) bytes of the pixels and up to 3 bytes to the end of the last dword
constexpr uint32_t raw_pitch_dwords(int R) { return (3u * (uint32_t) (kTileX + 2 * R) + 9u + 3u) / 4u; }
constexpr uint32_t raw_words(int R) { return ((uint32_t) (kTileY + 2 * R) * raw_pitch_dwords(R) + 3u) / 4u * 4u; }
constexpr uint32_t plane_words(int R) { return (uint32_t) (kTileY + 2 * R) * kRowBytes / 2u; }
constexpr uint32_t lds_bytes(int R) { return 4u * (raw_words(R) + plane_words(R) + kOutWords); }

constexpr int kMaxRows = kTileY + 2 * ksh::kMaxRadius;       // 80
constexpr int kStageTrips = (kMaxRows * raw_pitch_dwords(ksh::kMaxRadius) + kBlock - 1) / kBlock;
constexpr int kHaloTrips = (kMaxRows * 3 * 2 * ksh::kMaxRadius + kBlock - 1) / kBlock;
constexpr int kRowTrips = (kMaxRows * kRowBytes + kBlock - 1) / kBlock, kColumnTrips = kTileY * kRowBytes / kBlock, kStoreTrips = kTileY * 16 / kBlock;
static_assert(lds_bytes(ksh::kMaxRadius) <= 65536 && kOutPitch % 16 == 0 && kPieces <= 16 && (kTileY * kRowBytes) % kBlock == 0 && (kTileY * 16) % kBlock == 0 &&
              plane_words(1) % 4 == 0 && kRowBytes % 4 == 0, "the kernel's layout");

struct SharpenArgs {
    const uint8_t* src[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    ksh::Taps taps;
    uint32_t W, H, stride, out_stride;
    int32_t amount, threshold;
};

__global__ __launch_bounds__(kBlock) void k_sharpen(const SharpenArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_words[];
    const int32_t R = a.taps.radius;
    const uint32_t pitch = 4u * raw_pitch_dwords(R);                                            // of a staged row, in bytes
    uint8_t* const s_raw = reinterpret_cast<uint8_t*>(s_words);
    uint16_t* const s_plane = reinterpret_cast<uint16_t*>(s_words + raw_words(R));
    uint8_t* const s_out = reinterpret_cast<uint8_t*>(s_words + raw_words(R) + plane_words(R));

    const uint32_t tid = threadIdx.x;
    const uint32_t x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
    const uint32_t nx = a.W - x0 < (uint32_t) kTileX ? a.W - x0 : (uint32_t) kTileX, ny = a.H - y0 < (uint32_t) kTileY ? a.H - y0 : (uint32_t) kTileY;
    const uint32_t n_rows = ny + 2u * (uint32_t) R;                                             // staged row r is frame row clamp(y0 - R + r)
    // the pixels [fx, lx) of the frame are staged; `left` and `right` pixels of the halo lie beyond the frame
    const uint32_t fx = x0 > (uint32_t) R ? x0 - (uint32_t) R : 0u, lx = x0 + nx + (uint32_t) R < a.W ? x0 + nx + (uint32_t) R : a.W;
    const uint32_t left = fx + (uint32_t) R - x0, right = x0 + nx + (uint32_t) R - lx, span = lx - fx;
    const uint32_t lead_in = (3u * left + 3u) & ~3u;                                            // where a row's first dword goes: behind the left halo
    const uint8_t* const src = a.src[blockIdx.z];
    auto frame_row = [&](uint32_t r) -> const uint8_t* { return src + (size_t) ksh::clamped((int32_t) (y0 + r) - R, a.H) * a.stride + 3u * (size_t) fx; };
    // pixel fx of staged row r in LDS: (its address mod 4) bytes into the row's first dword
    auto staged = [&](uint32_t r) -> uint8_t* { return s_raw + r * pitch + lead_in + kbe_rows::shift_of(frame_row(r)); };

    // (1) the aligned dwords that hold a byte of the pixels [fx, lx) of a row: every one of them holds a byte of the row
    const uint32_t pitch_dwords = pitch / 4u;
    for (int trip = 0; trip < kStageTrips; trip++) {
        const uint32_t at = tid + (uint32_t) trip * kBlock, r = at / pitch_dwords, d = at - r * pitch_dwords;
        if (r >= n_rows) break;
        const kbe_rows::Fetch raw = kbe_rows::fetch_of(frame_row(r), span);
        if (d < raw.dwords) s_words[(r * pitch + lead_in) / 4u + d] = raw.base[d];
    }
    __syncthreads();
    // (1b) the same for every lane of the workgroup: only a tile at the frame's left or right border has such pixels
    if (left + right > 0u) {
        const uint32_t count = 3u * (left + right);
        for (int trip = 0; trip < kHaloTrips; trip++) {
            const uint32_t at = tid + (uint32_t) trip * kBlock, r = at / count, j = at - r * count;
            if (r >= n_rows) break;
            uint8_t* const row = staged(r);
            if (j < 3u * left) row[(int32_t) j - 3 * (int32_t) left] = row[j % 3u];
            else row[3u * span + (j - 3u * left)] = row[3u * (span - 1u) + (j - 3u * left) % 3u];
        }
        __syncthreads();
    }
    // byte b of the tile's row in staged row r: pixel x0 lies x0 - fx = R - left pixels behind pixel fx
    const uint32_t centre = 3u * ((uint32_t) R - left);
    // (2) the pass along the rows: value b of row r of the plane is channel b % 3 of column b / 3 of the tile
    for (int trip = 0; trip < kRowTrips; trip++) {
        const uint32_t at = tid + (uint32_t) trip * kBlock, r = at / kRowBytes, b = at - r * kRowBytes;
        if (r >= n_rows) break;
        if (b >= 3u * nx) continue;
        const uint8_t* const p = staged(r) + centre + b;
        s_plane[at] = (uint16_t) ksh::row_pass(a.taps, [&](int k) { return (uint32_t) p[3 * k]; });
    }
    __syncthreads();
    // (3) the pass down the columns and the mask; row ty of the tile starts (its address mod 16) bytes into its LDS row
    uint8_t* const dst = a.dst[blockIdx.z];
    for (int trip = 0; trip < kColumnTrips; trip++) {
        const uint32_t at = tid + (uint32_t) trip * kBlock, ty = at / kRowBytes, b = at - ty * kRowBytes;
        if (ty >= ny) break;
        if (b >= 3u * nx) continue;
        const uint16_t* const p = s_plane + (ty + (uint32_t) R) * kRowBytes + b;
        const uint32_t b16 = ksh::column_pass(a.taps, [&](int k) { return (uint32_t) p[k * kRowBytes]; });
        const uint32_t lead = kbe_rows::lead_of(dst + (size_t) (y0 + ty) * a.out_stride + 3u * (size_t) x0);
        s_out[ty * kOutPitch + lead + b] = (uint8_t) ksh::sharpened(staged(ty + (uint32_t) R)[centre + b], b16, a.amount, a.threshold);
    }
    __syncthreads();
    // (4) sixteen lanes per row of the tile, lane `piece` of them takes the bytes [16 piece, 16 piece + 16) of the LDS row
    for (int trip = 0; trip < kStoreTrips; trip++) {
        const uint32_t ty = (tid + (uint32_t) trip * kBlock) / 16u, at = 16u * (tid & 15u);
        if (ty >= ny) break;
        kbe_rows::store_tile_row(s_out + ty * kOutPitch, dst + (size_t) (y0 + ty) * a.out_stride + 3u * (size_t) x0, nx, at);
    }
}

}  // namespace

extern "C" {

KBE_SHARPEN_API int kbe_sharpen_abi_version(void)
{
    return KBE_SHARPEN_ABI_VERSION;
}

KBE_SHARPEN_API int kbe_sharpen_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, uint8_t* const* out_u8, int out_stride_bytes,
                                   const uint16_t* taps, int radius, int amount, int threshold, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!out_u8) what = "null out_u8";
    else if (!taps) what = "null taps";
    else if (n_frames < 1) what = "n_frames < 1";
    else if (!(W >= 1 && W <= kbe_rows::kMaxSide && H >= 1 && H <= kbe_rows::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (out_stride_bytes < 3 * W) what = "out_stride_bytes < 3 W";
    else if (!(radius >= 1 && radius <= ksh::kMaxRadius)) what = "radius outside 1..24";
    else if (!ksh::taps_ok(taps, radius)) what = "taps[0] + 2 (taps[1] + .. + taps[radius]) is not 32768";
    else if (!(amount >= 1 && amount <= ksh::kMaxAmount)) what = "amount outside 1..1024";
    else if (!(threshold >= 0 && threshold <= ksh::kMaxThreshold)) what = "threshold outside 0..255";
    for (int i = 0; !what && i < n_frames; i++)
        if (!frames_u8[i] || !out_u8[i]) what = frames_u8[i] ? "null element of out_u8" : "null element of frames_u8";
    if (what) return refuse("kbe_sharpen_u8", what);

    SharpenArgs a;
    for (int k = 0; k <= ksh::kMaxRadius; k++) a.taps.w[k] = k <= radius ? taps[k] : 0u;
    a.taps.radius = radius;
    a.W = (uint32_t) W;
    a.H = (uint32_t) H;
    a.stride = (uint32_t) stride_bytes;
    a.out_stride = (uint32_t) out_stride_bytes;
    a.amount = amount;
    a.threshold = threshold;
    const dim3 tiles(blocks_for((size_t) W, kTileX), blocks_for((size_t) H, kTileY));
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = launch_frames(n_frames, f0, kFramesPerLaunch);
        fill_slots(a.src, frames_u8, f0, nf);
        fill_slots(a.dst, out_u8, f0, nf);
        hipLaunchKernelGGL(k_sharpen, dim3(tiles.x, tiles.y, (unsigned) nf), dim3(kBlock), lds_bytes(radius), (hipStream_t) stream, a);
    }
    return launched("kbe_sharpen_u8");
}

}  // extern "C"
