// kbe_area.hip -- kbe_area_reduce_u8: frames that lie in HBM, reduced by the exact area average of kbe_area_block.h, for area.py
// (include/kbe_area.h).  The arithmetic is the header's accumulate() and rounded(), as they are; this file spreads the work over the chip.
//
// One workgroup takes a TILE of kTileX x kTileY target pixels of one frame (the frame is the grid's z), one thread per target pixel.  The
// sources a tile overlaps are at most ceil(tile * N / n) + 1 per axis, which has no bound of its own, so they pass through LDS in STRIPS of
// kStripRows rows of kStripPx pixels: the LDS is fixed, whatever the ratio.  A strip's rows are fetched as aligned dwords, a lane per dword
// and a row per step -- no 3-byte pixel is a byte-wide global load; the row's first pixel then lies 0..3 bytes into its LDS row.  Every thread
// adds what the strip holds of its own footprint (exact integer sums: the order of the strips does not matter).  The tile's bytes are put
// together in LDS at the output rows' own alignment modulo 16 and stored as 16-byte pieces, with dwords and single bytes only where a row's
// ends do not fill a piece; nothing outside a row's 3 w bytes is written.  The row fetch, the tile's row in LDS and its store are
// kbe_rows.h's, which the other tile kernels share.
//
// Every loop has a static bound (the strips of the tile's span, the rows and pixels of a strip); no kernel waits for another workgroup.  A
// thread walks its pixel's whole footprint, so the time per target pixel grows with (W / w)(H / h): meant for the few-fold reductions of
// the GIF route, correct for any.  Next to the encode it feeds this kernel is bandwidth-trivial; it is coalesced and not tuned further.
#include "kbe_area.h"
#include "kbe_area_block.h"
#include "kbe_host.h"

using namespace kbe;
using namespace kbe_area;

namespace {

using kbe_rows::kFramesPerLaunch;
constexpr int kTileX = 64, kTileY = 4;                      // one wave per target row of the tile
constexpr int kStripRows = 16, kStripDwords = kBlock;       // a lane per dword of a strip's row
constexpr int kStripPx = (4 * kStripDwords - 3) / 3;        // 340: 3 bytes of misalignment and 1020 of pixels fit the 1024
constexpr int kOutPitch = 3 * kTileX + 16;                  // a tile's row of 192 bytes, 0..15 bytes into its LDS row
static_assert(kTileX * kTileY == kBlock && kTileX == 64 && kOutPitch % 16 == 0 && 3 + 3 * kStripPx <= 4 * kStripDwords, "the kernel's layout");

struct AreaArgs {
    const uint8_t* src[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    Shape g;
    uint32_t stride, out_stride;
};

// a strip in LDS: row sy of the source starts `shift(sy)` bytes into row sy - y0
struct Strip {
    const uint8_t* bytes;
    const uint8_t* src;
    size_t stride;
    uint32_t x0, y0;
    struct Row {
        const uint8_t* p;
        uint32_t x0;
        __device__ __forceinline__ uint32_t operator()(uint32_t sx, int c) const { return p[3u * (sx - x0) + c]; }
    };
    __device__ __forceinline__ const uint8_t* first(uint32_t sy) const { return src + (size_t) sy * stride + 3u * (size_t) x0; }
    __device__ __forceinline__ Row row(uint32_t sy) const
    {
        return Row{bytes + (sy - y0) * (4u * kStripDwords) + kbe_rows::shift_of(first(sy)), x0};
    }
};

__global__ __launch_bounds__(kBlock) void k_area_reduce(const AreaArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_words[kStripRows * kStripDwords + kTileY * kOutPitch / 4];
    uint8_t* const s_out = reinterpret_cast<uint8_t*>(s_words + kStripRows * kStripDwords);

    const Shape g = a.g;
    const uint32_t tid = threadIdx.x, tx = tid & (kTileX - 1), ty = tid / kTileX;
    const uint32_t ox0 = blockIdx.x * kTileX, oy0 = blockIdx.y * kTileY;
    const uint32_t nx = g.w - ox0 < (uint32_t) kTileX ? g.w - ox0 : (uint32_t) kTileX, ny = g.h - oy0 < (uint32_t) kTileY ? g.h - oy0 : (uint32_t) kTileY;
    const uint32_t ox = ox0 + tx, oy = oy0 + ty;
    const bool mine = tx < nx && ty < ny;
    // the tile's span of the source (the same in every lane), and this thread's footprint in it
    const Window tile = {span_begin(ox0, g.W, g.w), span_end(ox0 + nx - 1u, g.W, g.w), span_begin(oy0, g.H, g.h), span_end(oy0 + ny - 1u, g.H, g.h)};
    const Window own = mine ? footprint(g, ox, oy) : Window{0u, 0u, 0u, 0u};
    Strip strip = {reinterpret_cast<const uint8_t*>(s_words), a.src[blockIdx.z], a.stride, 0u, 0u};

    uint64_t acc[3] = {0u, 0u, 0u};
    for (uint32_t y0 = tile.y0; y0 < tile.y1; y0 += kStripRows) {
        const uint32_t y1 = tile.y1 - y0 < (uint32_t) kStripRows ? tile.y1 : y0 + kStripRows;
        for (uint32_t x0 = tile.x0; x0 < tile.x1; x0 += kStripPx) {
            const uint32_t x1 = tile.x1 - x0 < (uint32_t) kStripPx ? tile.x1 : x0 + kStripPx;
            strip.x0 = x0;
            strip.y0 = y0;
            __syncthreads();                                           // (the strip before this one has been read)
            for (uint32_t sy = y0; sy < y1; sy++) {
                // the aligned dwords that hold a byte of pixels x0 .. x1 - 1 of row sy: every one of them holds a byte of the row
                const kbe_rows::Fetch row = kbe_rows::fetch_of(strip.first(sy), x1 - x0);
                if (tid < row.dwords) s_words[(sy - y0) * kStripDwords + tid] = row.base[tid];
            }
            __syncthreads();
            accumulate(g, ox, oy, intersect(own, Window{x0, x1, y0, y1}), strip, acc);
        }
    }

    // the tile's bytes at their rows' alignment: row ty starts (its address mod 16) bytes into its LDS row
    uint8_t* const row = a.dst[blockIdx.z] + (size_t) oy * a.out_stride + 3u * (size_t) ox0;
    if (mine) {
        const uint32_t lead = kbe_rows::lead_of(row);
        for (int c = 0; c < 3; c++) s_out[ty * kOutPitch + lead + 3u * tx + c] = rounded(acc[c], g);
    }
    __syncthreads();
    if (ty < ny) kbe_rows::store_tile_row(s_out + ty * kOutPitch, row, nx, 16u * tx);             // lane tx takes the piece [16 tx, 16 tx + 16)
}

}  // namespace

extern "C" {

KBE_AREA_API int kbe_area_abi_version(void)
{
    return KBE_AREA_ABI_VERSION;
}

KBE_AREA_API int kbe_area_reduce_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, uint8_t* const* out_u8, int w, int h, int out_stride_bytes,
                                    kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!out_u8) what = "null out_u8";
    else if (n_frames < 1) what = "n_frames < 1";
    else if (!(W >= 1 && W <= kMaxSide && H >= 1 && H <= kMaxSide)) what = "W or H outside 1..65535";
    else if (!(w >= 1 && w <= W)) what = "w outside 1..W: the entry only reduces";
    else if (!(h >= 1 && h <= H)) what = "h outside 1..H: the entry only reduces";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (out_stride_bytes < 3 * w) what = "out_stride_bytes < 3 w";
    for (int i = 0; !what && i < n_frames; i++)
        if (!frames_u8[i] || !out_u8[i]) what = frames_u8[i] ? "null element of out_u8" : "null element of frames_u8";
    if (what) return refuse("kbe_area_reduce_u8", what);

    AreaArgs a;
    a.g = Shape{(uint32_t) W, (uint32_t) H, (uint32_t) w, (uint32_t) h};
    a.stride = (uint32_t) stride_bytes;
    a.out_stride = (uint32_t) out_stride_bytes;
    const dim3 tiles(blocks_for((size_t) w, kTileX), blocks_for((size_t) h, kTileY));
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = launch_frames(n_frames, f0, kFramesPerLaunch);
        fill_slots(a.src, frames_u8, f0, nf);
        fill_slots(a.dst, out_u8, f0, nf);
        hipLaunchKernelGGL(k_area_reduce, dim3(tiles.x, tiles.y, (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_area_reduce_u8");
}

}  // extern "C"
