// kbe_dof.hip -- kbe_dof_u8: raw frames that lie in HBM, blurred by the depth of every pixel, for dof.py (include/kbe_dof.h).  The arithmetic
// is kbe_dof_block.h's radius(), extent(), covers(), add() and rounded(), as they are; this file spreads the work over the chip, in the shape of
// k_crop_area (kbe_crop_area.hip), which stays as it is.
//
// One workgroup takes a TILE of kTileX x kTileY target pixels of one frame (the frame is the grid's z), one thread per target pixel.  The
// tile and a halo of R = max_radius pixels around it, as far as the frame goes, are staged in LDS:
//   (0) the rows' colour bytes are fetched as aligned dwords, a lane per dword and a wave per row; the row's first pixel lies 0..3 bytes into
//       its LDS row;
//   (1) every staged pixel becomes ONE word -- its three bytes and, in the top byte, its radius, computed here once -- and its depth is kept
//       beside it as the fp32 it is, so that z(q) <= z(p) stays the comparison of the definition.  A cell outside the frame gets radius 0:
//       at a distance of 1 or more it never contributes.  The largest radius m among the staged pixels is found on the way;
//   (2) every thread walks the window |dy| <= m, dx^2 + dy^2 <= m^2 around its pixel: no sample spreads further than its own radius, so
//       the rest of the (2 R + 1)^2 window cannot contribute.  m is the same in the whole workgroup.  A tile of an in-focus region, and every
//       tile at aperture 0, therefore costs a copy.
// The tile's bytes are put together in LDS at the output rows' own alignment modulo 16 and stored as 16-byte pieces, with dwords and single
// bytes only where a row's ends do not fill a piece; nothing outside a row's 3 W bytes is written.  The row fetch's arithmetic, the tile's
// row in LDS and its store are kbe_rows.h's, which k_area_reduce and k_crop_area run too.
//
// Every loop has a static bound (the rows and dwords of the staged window, at most 2 R + 1 steps per axis of the walk); no workgroup waits for
// another.  LDS: 96 x 48 cells of 8 bytes (36 KiB, whatever R is) and 13.9 KiB of raw rows, which the output rows reuse: 51 144 bytes of a CU's
// 160 KiB.  Three workgroups would fit by LDS; the 16 waves of a workgroup let two be resident on a CU's 32 wave slots.
#include <float.h>

#include "kbe_dof.h"
#include "kbe_dof_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace kdof = kbe_dof;

namespace {

using kbe_rows::kFramesPerLaunch;
constexpr int kTileX = 64, kTileY = 16;                     // one wave per target row of the tile
constexpr int kThreads = kTileX * kTileY, kWaves = kThreads / 64;
constexpr int kCellsX = kTileX + 2 * kdof::kMaxRadius, kCellsY = kTileY + 2 * kdof::kMaxRadius;      // 96 x 48 staged pixels
constexpr int kRawDwords = (3 + 3 * kCellsX + 3) / 4 + 1;   // 74: 3 bytes of misalignment and 288 of pixels fit 73 dwords; 74 keeps rows apart by an even count
constexpr int kRawWords = kCellsY * kRawDwords;
constexpr int kOutPitch = 3 * kTileX + 16;                  // a tile's row of 192 bytes, 0..15 bytes into its LDS row
static_assert(kTileX == 64 && kThreads <= 1024 && kOutPitch % 16 == 0 && kTileY * kOutPitch <= 4 * kRawWords && kRawWords % 4 == 0 && 3 + 3 * kCellsX <= 4 * kRawDwords, "the kernel's layout");

struct DofArgs {
    const uint8_t* src[kFramesPerLaunch];
    const float* depth[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    float focus[kFramesPerLaunch];
    float aperture;
    int R;
    uint32_t W, H, stride, depth_stride, out_stride;
};

__global__ __launch_bounds__(kThreads) void k_dof(const DofArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[kRawWords];             // (0); after (1) the tile's output rows
    __shared__ uint32_t s_px[kCellsY * kCellsX];
    __shared__ float s_z[kCellsY * kCellsX];
    __shared__ uint32_t s_weight[kdof::kMaxRadius + 1];
    __shared__ uint32_t s_max;
    uint8_t* const s_out = reinterpret_cast<uint8_t*>(s_raw);

    const int R = a.R;
    const uint32_t tid = threadIdx.x, tx = tid & (kTileX - 1), ty = tid / kTileX;         // ty is the thread's wave
    const uint32_t ox0 = blockIdx.x * kTileX, oy0 = blockIdx.y * kTileY;
    const uint32_t nx = a.W - ox0 < (uint32_t) kTileX ? a.W - ox0 : (uint32_t) kTileX, ny = a.H - oy0 < (uint32_t) kTileY ? a.H - oy0 : (uint32_t) kTileY;
    const bool mine = tx < nx && ty < ny;
    // the staged window: cell (lx, ly) is pixel (ox0 - R + lx, oy0 - R + ly); [cx0, cx1) x [cy0, cy1) of it lies inside the frame
    const int wx = kTileX + 2 * R, wy = kTileY + 2 * R;
    const int px0 = (int) ox0 - R, py0 = (int) oy0 - R;
    const uint32_t fx0 = px0 < 0 ? 0u : (uint32_t) px0, fy0 = py0 < 0 ? 0u : (uint32_t) py0;                 // the first pixel and row fetched
    const uint32_t fx1 = ox0 + nx + (uint32_t) R < a.W ? ox0 + nx + (uint32_t) R : a.W, fy1 = oy0 + ny + (uint32_t) R < a.H ? oy0 + ny + (uint32_t) R : a.H;
    const uint8_t* const src = a.src[blockIdx.z];
    const float* const depth = a.depth[blockIdx.z];
    const float zf = a.focus[blockIdx.z], A = a.aperture;

    if (tid <= (uint32_t) kdof::kMaxRadius) s_weight[tid] = kdof::kWeight.w[tid];
    if (tid == 0u) s_max = 0u;
    // (0) the aligned dwords that hold a byte of pixels fx0 .. fx1 - 1 of row fy: every one of them holds a byte of the row
    for (uint32_t fy = fy0 + ty; fy < fy1; fy += kWaves) {
        const kbe_rows::Fetch row = kbe_rows::fetch_of(src + (size_t) fy * a.stride + 3u * (size_t) fx0, fx1 - fx0);         // at most 73 dwords
        for (uint32_t d = tx; d < row.dwords; d += 64u) s_raw[(fy - fy0) * kRawDwords + d] = row.base[d];
    }
    __syncthreads();
    // (1) the cells: a wave per row of the window
    uint32_t largest = 0u;
    for (int ly = (int) ty; ly < wy; ly += kWaves) {
        const int y = py0 + ly;
        const bool row_in = y >= (int) fy0 && y < (int) fy1;
        const uint8_t* raw_row = nullptr;
        if (row_in) {
            const uint8_t* const first = src + (size_t) y * a.stride + 3u * (size_t) fx0;
            raw_row = reinterpret_cast<const uint8_t*>(s_raw + ((uint32_t) y - fy0) * kRawDwords) + kbe_rows::shift_of(first);
        }
        for (int lx = (int) tx; lx < wx; lx += 64) {
            const int x = px0 + lx;
            uint32_t word = 0u;
            float z = 0.0f;
            if (row_in && x >= (int) fx0 && x < (int) fx1) {
                z = depth[(size_t) y * a.depth_stride + (size_t) x];
                const uint8_t* const p = raw_row + 3u * ((uint32_t) x - fx0);
                const uint32_t r = kdof::radius(z, zf, A, R);
                word = (uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16 | r << 24;
                largest = r > largest ? r : largest;
            }
            s_px[ly * kCellsX + lx] = word;
            s_z[ly * kCellsX + lx] = z;
        }
    }
    if (largest > 0u) atomicMax(&s_max, largest);
    __syncthreads();
    // (2)
    const int m = (int) s_max;
    uint8_t* const row = a.dst[blockIdx.z] + (size_t) (oy0 + ty) * a.out_stride + 3u * (size_t) ox0;         // the output row of this thread's wave
    if (mine) {
        const int cell = ((int) ty + R) * kCellsX + (int) tx + R;
        const uint32_t own = s_px[cell], rp = own >> 24;
        const float zp = s_z[cell];
        kdof::Sums s = {0u, {0u, 0u, 0u}};
        kdof::add(s, s_weight[rp], own & 255u, own >> 8 & 255u, own >> 16 & 255u);
        for (int dy = -m; dy <= m; dy++) {
            int reach = m;                                             // the widest dx with dx^2 + dy^2 <= m^2
            while (reach * reach + dy * dy > m * m) reach--;
            for (int dx = -reach; dx <= reach; dx++) {
                const uint32_t q = s_px[cell + dy * kCellsX + dx], rq = q >> 24;
                if (rq == 0u || (dx == 0 && dy == 0)) continue;        // (radius 0 reaches only itself; the target has been added)
                const uint32_t e = kdof::extent(rq, s_z[cell + dy * kCellsX + dx], rp, zp);
                if (kdof::covers(dx, dy, e)) kdof::add(s, s_weight[e], q & 255u, q >> 8 & 255u, q >> 16 & 255u);
            }
        }
        // the tile's bytes at their rows' alignment: row ty starts (its address mod 16) bytes into its LDS row (the raw rows are done with)
        const uint32_t lead = kbe_rows::lead_of(row);
        for (int c = 0; c < 3; c++) s_out[ty * kOutPitch + lead + 3u * tx + c] = (uint8_t) kdof::rounded(s.v[c], s.w);
    }
    __syncthreads();
    if (ty < ny) kbe_rows::store_tile_row(s_out + ty * kOutPitch, row, nx, 16u * tx);             // lane tx takes the piece [16 tx, 16 tx + 16)
}

}  // namespace

extern "C" {

KBE_DOF_API int kbe_dof_abi_version(void)
{
    return KBE_DOF_ABI_VERSION;
}

KBE_DOF_API int kbe_dof_u8(const uint8_t* const* frames_u8, const float* const* depth_f32, int n_frames, int W, int H, int stride_bytes,
                           int depth_stride_floats, const double* focus, double aperture, int max_radius, uint8_t* const* out_u8,
                           int out_stride_bytes, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!depth_f32) what = "null depth_f32";
    else if (!focus) what = "null focus";
    else if (!out_u8) what = "null out_u8";
    else if (n_frames < 1) what = "n_frames < 1";
    else if (!(W >= 1 && W <= kdof::kMaxSide && H >= 1 && H <= kdof::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (depth_stride_floats < W) what = "depth_stride_floats < W";
    else if (out_stride_bytes < 3 * W) what = "out_stride_bytes < 3 W";
    else if (!(max_radius >= 0 && max_radius <= kdof::kMaxRadius)) what = "max_radius outside 0..16";
    else if (!(aperture >= 0.0 && (double) (float) aperture <= (double) FLT_MAX)) what = "aperture is not a finite number >= 0";
    for (int i = 0; !what && i < n_frames; i++) {
        if (!frames_u8[i]) what = "null element of frames_u8";
        else if (!depth_f32[i]) what = "null element of depth_f32";
        else if (!out_u8[i]) what = "null element of out_u8";
        else if (!((float) focus[i] > 0.0f && (float) focus[i] <= FLT_MAX)) what = "an element of focus is not a finite number > 0";
    }
    // a gather in place is wrong: no output may share a byte with a source frame or a depth plane of the call
    if (!what) {
        const uintptr_t src_bytes = frame_extent(H, stride_bytes, 3u * (uintptr_t) W), out_bytes = frame_extent(H, out_stride_bytes, 3u * (uintptr_t) W);
        const uintptr_t depth_bytes = frame_extent(H, 4u * (uintptr_t) depth_stride_floats, 4u * (uintptr_t) W);
        if (any_overlap(out_u8, n_frames, out_bytes, frames_u8, n_frames, src_bytes)) what = "an element of out_u8 overlaps a source frame";
        else if (any_overlap(out_u8, n_frames, out_bytes, depth_f32, n_frames, depth_bytes)) what = "an element of out_u8 overlaps a depth plane";
    }
    if (what) return refuse("kbe_dof_u8", what);

    DofArgs a;
    a.aperture = (float) aperture;
    a.R = max_radius;
    a.W = (uint32_t) W;
    a.H = (uint32_t) H;
    a.stride = (uint32_t) stride_bytes;
    a.depth_stride = (uint32_t) depth_stride_floats;
    a.out_stride = (uint32_t) out_stride_bytes;
    const dim3 tiles(blocks_for((size_t) W, kTileX), blocks_for((size_t) H, kTileY));
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = launch_frames(n_frames, f0, kFramesPerLaunch);
        fill_slots(a.src, frames_u8, f0, nf);
        fill_slots(a.depth, depth_f32, f0, nf);
        fill_slots(a.dst, out_u8, f0, nf);
        for (int i = 0; i < kFramesPerLaunch; i++) a.focus[i] = i < nf ? (float) focus[f0 + i] : 1.0f;
        hipLaunchKernelGGL(k_dof, dim3(tiles.x, tiles.y, (unsigned) nf), dim3(kThreads), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_dof_u8");
}

}  // extern "C"
