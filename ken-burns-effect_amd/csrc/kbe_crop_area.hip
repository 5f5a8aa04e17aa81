// kbe_crop_area.hip -- kbe_crop_area_u8: raw frames that lie in HBM, their centred crop reduced by the exact area average, for crop_area.py
// (include/kbe_crop_area.h).  The arithmetic is kbe_crop_area_block.h's patch and kbe_area_block.h's accumulate() and rounded(), as they
// are; this file spreads the work over the chip, in the shape of k_area_reduce (kbe_area.hip), which stays as it is.
//
// One workgroup takes a TILE of kTileX x kTileY target pixels of one frame (the frame is the grid's z), one thread per target pixel.  The
// PATCH pixels a tile overlaps pass through LDS in STRIPS of at most kStripRows rows of kStripPx pixels, and under a strip of the patch lies
// its span of the RAW frame: one row and one pixel more (the second taps of a half-pixel start).  Per strip
//   (0) the raw rows are fetched as aligned dwords, a lane per dword and a row per step; the row's first pixel lies 0..3 bytes into its LDS row;
//   (1) the strip's patch bytes are made ONCE in LDS from the staged raw rows: a thread owns byte columns and walks down the rows, the
//       bottom taps of one row being the top taps of the next.  A crop that starts on whole pixels on both axes IS the raw rectangle: the
//       step is skipped and (2) reads the staged raw rows.  The test is uniform over the launch;
//   (2) every thread adds what the strip holds of its own footprint (exact integer sums: the order of the strips does not matter).
// The tile's bytes are put together in LDS at the output rows' own alignment modulo 16 and stored as 16-byte pieces, with dwords and single
// bytes only where a row's ends do not fill a piece; nothing outside a row's 3 w bytes is written.  The row fetch, the tile's row in LDS
// and its store are kbe_rows.h's, which k_area_reduce runs too.
//
// Every loop has a static bound (the strips of the tile's span, the rows and byte columns of a strip); no kernel waits for another
// workgroup.  A thread walks its pixel's whole footprint, so the time per target pixel grows with (cw / w)(ch / h): meant for the few-fold
// reductions of a delivered video, correct for any.
#include "kbe_crop_area.h"
#include "kbe_crop_area_block.h"
#include "kbe_host.h"

using namespace kbe;
using namespace kbe_area;
namespace kca = kbe_crop_area;

namespace {

using kbe_rows::kFramesPerLaunch;
constexpr int kTileX = 64, kTileY = 4;                      // one wave per target row of the tile
constexpr int kRawDwords = kBlock;                          // a lane per dword of a staged raw row
constexpr int kRawPx = (4 * kRawDwords - 3) / 3;            // 340: 3 bytes of misalignment and 1020 of pixels fit the 1024
constexpr int kStripRows = 16, kStripPx = kRawPx - 1;       // a strip of the patch; its raw span is one row and one pixel more
constexpr int kRawRows = kStripRows + 1;
constexpr int kPatchPitch = (3 * kStripPx + 3) / 4 * 4;     // 1020 bytes
constexpr int kPatchCols = (3 * kStripPx + kBlock - 1) / kBlock;      // byte columns of a strip per thread: 4
constexpr int kOutPitch = 3 * kTileX + 16;                  // a tile's row of 192 bytes, 0..15 bytes into its LDS row
constexpr int kRawWords = kRawRows * kRawDwords, kPatchWords = kStripRows * kPatchPitch / 4;
static_assert(kTileX * kTileY == kBlock && kTileX == 64 && kOutPitch % 16 == 0 && 3 + 3 * (kStripPx + 1) <= 4 * kRawDwords && (kRawWords + kPatchWords) % 4 == 0, "the kernel's layout");

struct CropAreaArgs {
    const uint8_t* src[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    kca::Crop k;
    uint32_t w, h, stride, out_stride;
};

// the staged raw rows: raw row ry, from its pixel rx0 on, starts `shift(ry)` bytes into LDS row ry - ry0
struct Raw {
    const uint8_t* bytes;
    const uint8_t* src;
    size_t stride;
    uint32_t rx0, ry0;
    __device__ __forceinline__ const uint8_t* first(uint32_t ry) const { return src + (size_t) ry * stride + 3u * (size_t) rx0; }
    __device__ __forceinline__ const uint8_t* at(uint32_t ry) const { return bytes + (ry - ry0) * (4u * kRawDwords) + kbe_rows::shift_of(first(ry)); }
};

// the Sources of accumulate(): a strip of the patch from pixel (x0, y0) on -- made in LDS, or the staged raw rows themselves
struct Row {
    const uint8_t* p;
    uint32_t x0;
    __device__ __forceinline__ uint32_t operator()(uint32_t sx, int c) const { return p[3u * (sx - x0) + c]; }
};

struct MadeStrip {
    const uint8_t* bytes;
    uint32_t x0, y0;
    __device__ __forceinline__ Row row(uint32_t sy) const { return Row{bytes + (sy - y0) * kPatchPitch, x0}; }
};

struct RawStrip {
    Raw raw;
    uint32_t x0, ipy;
    __device__ __forceinline__ Row row(uint32_t sy) const { return Row{raw.at(ipy + sy), x0}; }
};

__global__ __launch_bounds__(kBlock) void k_crop_area(const CropAreaArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_words[kRawWords + kPatchWords + kTileY * kOutPitch / 4];
    uint8_t* const s_patch = reinterpret_cast<uint8_t*>(s_words + kRawWords);
    uint8_t* const s_out = reinterpret_cast<uint8_t*>(s_words + kRawWords + kPatchWords);

    const kca::Crop k = a.k;
    const Shape g = {k.cw, k.ch, a.w, a.h};
    const uint32_t tid = threadIdx.x, tx = tid & (kTileX - 1), ty = tid / kTileX;
    const uint32_t ox0 = blockIdx.x * kTileX, oy0 = blockIdx.y * kTileY;
    const uint32_t nx = g.w - ox0 < (uint32_t) kTileX ? g.w - ox0 : (uint32_t) kTileX, ny = g.h - oy0 < (uint32_t) kTileY ? g.h - oy0 : (uint32_t) kTileY;
    const uint32_t ox = ox0 + tx, oy = oy0 + ty;
    const bool mine = tx < nx && ty < ny;
    // the tile's span of the patch (the same in every lane), and this thread's footprint in it
    const Window tile = {span_begin(ox0, g.W, g.w), span_end(ox0 + nx - 1u, g.W, g.w), span_begin(oy0, g.H, g.h), span_end(oy0 + ny - 1u, g.H, g.h)};
    const Window own = mine ? footprint(g, ox, oy) : Window{0u, 0u, 0u, 0u};
    // where the patch lies in the raw frame (uniform over the launch)
    const uint32_t ipx = kca::start(k.W, k.cw), ipy = kca::start(k.H, k.ch);
    const uint32_t hx = kca::half(k.W, k.cw) ? 1u : 0u, hy = kca::half(k.H, k.ch) ? 1u : 0u;
    const bool whole = kca::whole(k);
    Raw raw = {reinterpret_cast<const uint8_t*>(s_words), a.src[blockIdx.z], a.stride, 0u, 0u};

    uint64_t acc[3] = {0u, 0u, 0u};
    for (uint32_t y0 = tile.y0; y0 < tile.y1; y0 += kStripRows) {
        const uint32_t y1 = tile.y1 - y0 < (uint32_t) kStripRows ? tile.y1 : y0 + kStripRows;
        for (uint32_t x0 = tile.x0; x0 < tile.x1; x0 += kStripPx) {
            const uint32_t x1 = tile.x1 - x0 < (uint32_t) kStripPx ? tile.x1 : x0 + kStripPx;
            // the raw rectangle under the strip [x0, x1) x [y0, y1) of the patch: its second taps too, as far as the frame goes
            const uint32_t rx0 = ipx + x0, rx1 = ipx + x1 + hx < k.W ? ipx + x1 + hx : k.W;            // at most kStripPx + 1 pixels
            const uint32_t ry0 = ipy + y0, ry1 = ipy + y1 + hy < k.H ? ipy + y1 + hy : k.H;            // at most kRawRows rows
            raw.rx0 = rx0;
            raw.ry0 = ry0;
            __syncthreads();                                           // (the strip before this one has been read)
            // (0) the aligned dwords that hold a byte of pixels rx0 .. rx1 - 1 of raw row ry: every one of them holds a byte of the row
            for (uint32_t ry = ry0; ry < ry1; ry++) {
                const kbe_rows::Fetch row = kbe_rows::fetch_of(raw.first(ry), rx1 - rx0);
                if (tid < row.dwords) s_words[(ry - ry0) * kRawDwords + tid] = row.base[tid];
            }
            __syncthreads();
            const Window in = intersect(own, Window{x0, x1, y0, y1});
            if (whole) {                                               // uniform: the raw strip is the patch
                accumulate(g, ox, oy, in, RawStrip{raw, x0, ipy}, acc);
                continue;
            }
            // (1) the strip's patch bytes: byte column b of the strip is channel b % 3 of patch pixel x0 + b / 3
            const uint32_t n_bytes = 3u * (x1 - x0), n_rows = y1 - y0;
            for (int j = 0; j < kPatchCols; j++) {
                const uint32_t b = tid + (uint32_t) j * kBlock;
                if (b >= n_bytes) break;
                const uint32_t px = b / 3u, c = b - 3u * px;
                const uint32_t o0 = 3u * (kca::tap0(k.W, k.cw, x0 + px) - rx0) + c, o1 = 3u * (kca::tap1(k.W, k.cw, x0 + px) - rx0) + c;
                uint32_t t0 = 0u, t1 = 0u;
                for (uint32_t pr = 0; pr < n_rows; pr++) {
                    if (pr == 0u || !hy) {                             // (with a half-pixel start down the frame the last row's bottom taps are kept)
                        const uint8_t* const r = raw.at(kca::tap0(k.H, k.ch, y0 + pr));
                        t0 = r[o0];
                        t1 = r[o1];
                    }
                    uint32_t u0 = t0, u1 = t1;
                    if (hy) {
                        const uint8_t* const r = raw.at(kca::tap1(k.H, k.ch, y0 + pr));
                        u0 = r[o0];
                        u1 = r[o1];
                    }
                    s_patch[pr * kPatchPitch + b] = (uint8_t) kca::patch_value(t0, t1, u0, u1);
                    t0 = u0;
                    t1 = u1;
                }
            }
            __syncthreads();
            // (2)
            accumulate(g, ox, oy, in, MadeStrip{s_patch, x0, y0}, acc);
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

KBE_CROP_AREA_API int kbe_crop_area_abi_version(void)
{
    return KBE_CROP_AREA_ABI_VERSION;
}

KBE_CROP_AREA_API int kbe_crop_area_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int crop_w, int crop_h, uint8_t* const* out_u8, int w, int h,
                                       int out_stride_bytes, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!out_u8) what = "null out_u8";
    else if (n_frames < 1) what = "n_frames < 1";
    else if (!(W >= 1 && W <= kMaxSide && H >= 1 && H <= kMaxSide)) what = "W or H outside 1..65535";
    else if (!(crop_w >= 1 && crop_w <= W)) what = "crop_w outside 1..W";
    else if (!(crop_h >= 1 && crop_h <= H)) what = "crop_h outside 1..H";
    else if (!(w >= 1 && w <= crop_w)) what = "w outside 1..crop_w: the entry only reduces";
    else if (!(h >= 1 && h <= crop_h)) what = "h outside 1..crop_h: the entry only reduces";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (out_stride_bytes < 3 * w) what = "out_stride_bytes < 3 w";
    for (int i = 0; !what && i < n_frames; i++)
        if (!frames_u8[i] || !out_u8[i]) what = frames_u8[i] ? "null element of out_u8" : "null element of frames_u8";
    if (what) return refuse("kbe_crop_area_u8", what);

    CropAreaArgs a;
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
        hipLaunchKernelGGL(k_crop_area, dim3(tiles.x, tiles.y, (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_crop_area_u8");
}

}  // extern "C"
