// kbe_yuv.hip -- kbe_yuv420_u8: every frame of 3-byte pixels that lies in HBM as planar Y'CbCr 4:2:0, BT.601 at limited range, for yuv.py
// (include/kbe_yuv.h).  The arithmetic is kbe_yuv_block.h's run(), shift_in() and store_piece(), as they are; this file spreads the work over
// the chip.  A streaming kernel: it reads 3 W H bytes and writes 1.5 W H per frame, and nothing is read twice.
//
// A wave takes one ROW PAIR of a frame -- the rows 2 cy and 2 cy + 1, one row of chroma cells -- and the four waves of a workgroup take four
// row pairs.  A lane takes a run of 16 pixels, 8 cells, of the pair: 48 source bytes of each row, which begin at the row's own alignment,
// b = 0..3 bytes into an aligned dword.  The lane loads the 13 aligned dwords that hold them -- twelve as three 16-byte pieces at a dword's
// alignment, which the chip's global loads take, and the thirteenth on its own; at a row's two ends dword by dword, and only the dwords
// that hold a byte of the row: no address outside a row's dwords is touched -- and cuts its bytes out with a funnel shift by bytes.  No register
// is indexed by a variable.  A row wider than 1024 pixels is taken in several trips of the wave along it.
//
// The lane's results are 16 bytes of each Y row and 8 bytes of the Cb and of the Cr row.  The four streams lie at four alignments of their
// own, m = 0..3 bytes beyond a multiple of 4.  Every lane fetches the last dword its left neighbour made for a stream (a lane shuffle; the
// first lane of a trip takes it from the trip before, through a scalar register), moves its own dwords up by m bytes and stores ALIGNED
// dwords -- 16 and 8 bytes at once inside a stream --; the first lane of a row pair stores the stream's first 4 - m bytes and the last one
// its last m bytes one by one.  Nothing outside a plane's own bytes is stored.  A row of odd width ends in a cell of one column and a frame
// of odd height in a row of cells of one row: the pixel beside the missing one is taken twice, which is the definition's n = 2 and n = 1.
//
// The pointer tables travel as kernel arguments: a launch carries kFramesPerLaunch = 12 frames (the grid's z).  The only loop is the trips
// along a row; no workgroup waits for another; no LDS, no scratch.
#include "kbe_yuv.h"
#include "kbe_yuv_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace ky = kbe_yuv;

namespace {

constexpr int kFramesPerLaunch = KBE_YUV_FRAMES_PER_LAUNCH;
constexpr int kRowPairs = 4;                                // one wave per row pair
constexpr int kLanes = 64;
static_assert(kRowPairs * kLanes == kBlock && kFramesPerLaunch == kbe_rows::kFramesPerLaunch && ky::kFlagBGR == KBE_YUV_BGR, "the kernel's layout");

using kbe_rows::Dwords4;

struct YuvArgs {
    const uint8_t* src[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    ky::Coef k;
    uint32_t W, H, stride;
};

// the 13 aligned dwords around the 48 bytes of a row that begin at `first`, b bytes into the first of them: inside the row, where every one
// of them holds a byte of it, as three 16-byte pieces and a dword
__device__ __forceinline__ void load_inside(const uint8_t* first, uint32_t b, uint32_t (&x)[ky::kRunDwords + 1])
{
    const uint32_t* const dwords = reinterpret_cast<const uint32_t*>(first - b);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const Dwords4 four = reinterpret_cast<const Dwords4*>(dwords)[q];
        x[4 * q] = four.x, x[4 * q + 1] = four.y, x[4 * q + 2] = four.z, x[4 * q + 3] = four.w;
    }
    x[ky::kRunDwords] = dwords[ky::kRunDwords];
}

// ... and at a row's two ends: dword by dword, and only those that hold a byte of the row
__device__ __forceinline__ void load_at_an_end(const uint8_t* first, uint32_t b, int j0, int row_bytes, uint32_t (&x)[ky::kRunDwords + 1])
{
    const uint32_t* const dwords = reinterpret_cast<const uint32_t*>(first - b);
#pragma unroll
    for (int k = 0; k <= ky::kRunDwords; k++) x[k] = kbe_rows::dword_holds_a_byte<ky::kRunDwords>(j0, b, k, row_bytes) ? dwords[k] : 0u;
}

// the value of the lane to the left; the first lane's is `carry`
__device__ __forceinline__ uint32_t from_the_left(uint32_t v, uint32_t lane, uint32_t carry)
{
    const uint32_t left = (uint32_t) __shfl_up((int) v, 1, kLanes);
    return lane == 0u ? carry : left;
}

__global__ __launch_bounds__(kBlock) void k_yuv420(const YuvArgs a)
{
    const uint32_t lane = threadIdx.x & (kLanes - 1), cy = blockIdx.x * kRowPairs + threadIdx.x / kLanes;
    const int W = (int) a.W, H = (int) a.H, cw = (W + 1) / 2, ch = (H + 1) / 2, row_bytes = 3 * W;
    if ((int) cy >= ch) return;                                                               // (a whole wave)
    const bool two = 2 * (int) cy + 1 < H;
    const uint8_t* const top = a.src[blockIdx.z] + (size_t) (2u * cy) * a.stride;
    uint8_t* const out = a.dst[blockIdx.z];
    ky::Streams s;
    s.ytop = out + (size_t) (2u * cy) * (size_t) W;
    s.ybot = two ? s.ytop + W : nullptr;
    s.cb = out + (size_t) W * (size_t) H + (size_t) cy * (size_t) cw;
    s.cr = s.cb + (size_t) cw * (size_t) ch;
    s.m_ytop = (uint32_t) ((uintptr_t) s.ytop & 3u), s.m_ybot = (uint32_t) ((uintptr_t) (s.ytop + W) & 3u);
    s.m_cb = (uint32_t) ((uintptr_t) s.cb & 3u), s.m_cr = (uint32_t) ((uintptr_t) s.cr & 3u);

    const int lanes = (W + ky::kRun - 1) / ky::kRun;
    uint32_t carry_ytop = 0u, carry_ybot = 0u, carry_cb = 0u, carry_cr = 0u;
    for (int g0 = 0; g0 < lanes; g0 += kLanes) {                                              // (every lane of the wave stays for the shuffles)
        const int g = g0 + (int) lane, j0 = 4 * ky::kRunDwords * g, x0 = ky::kRun * g;
        const bool live = g < lanes;
        // (both rows' loads are issued before either is waited for)
        const uint8_t* const first_top = top + j0;
        const uint8_t* const first_bot = first_top + (two ? a.stride : 0u);
        const uint32_t b_top = (uint32_t) ((uintptr_t) first_top & 3u), b_bot = (uint32_t) ((uintptr_t) first_bot & 3u);
        uint32_t xt[ky::kRunDwords + 1], xb[ky::kRunDwords + 1];
        if (live && kbe_rows::all_dwords_hold_a_byte<ky::kRunDwords>(j0, row_bytes)) {
            load_inside(first_top, b_top, xt);
            if (two) load_inside(first_bot, b_bot, xb);
        } else if (live) {
            load_at_an_end(first_top, b_top, j0, row_bytes, xt);
            if (two) load_at_an_end(first_bot, b_bot, j0, row_bytes, xb);
        } else {
#pragma unroll
            for (int k = 0; k <= ky::kRunDwords; k++) xt[k] = xb[k] = 0u;
        }
        if (!two) {                                                                            // (the last row of an odd height: it is its own bottom row)
#pragma unroll
            for (int k = 0; k <= ky::kRunDwords; k++) xb[k] = xt[k];
        }
        uint32_t t[ky::kRunDwords], b[ky::kRunDwords];
        ky::realign<ky::kRunDwords>(xt, b_top, t);
        ky::realign<ky::kRunDwords>(xb, b_bot, b);
        const int lone = (W & 1) && W - 1 >= x0 && W - 1 < x0 + ky::kRun ? (int) ((W - 1 - x0) / 2) : -1;
        uint32_t ytop[4], ybot[4], cb[2], cr[2];
        ky::run(t, b, lone, a.k, ytop, ybot, cb, cr);
        const uint32_t prev_ytop = from_the_left(ytop[3], lane, carry_ytop), prev_ybot = from_the_left(ybot[3], lane, carry_ybot);
        const uint32_t prev_cb = from_the_left(cb[1], lane, carry_cb), prev_cr = from_the_left(cr[1], lane, carry_cr);
        carry_ytop = __builtin_amdgcn_readlane(ytop[3], kLanes - 1), carry_ybot = __builtin_amdgcn_readlane(ybot[3], kLanes - 1);
        carry_cb = __builtin_amdgcn_readlane(cb[1], kLanes - 1), carry_cr = __builtin_amdgcn_readlane(cr[1], kLanes - 1);
        if (live) ky::store_run(s, g, W, cw, ytop, ybot, cb, cr, prev_ytop, prev_ybot, prev_cb, prev_cr);
    }
}

}  // namespace

extern "C" {

KBE_YUV_API int kbe_yuv_abi_version(void)
{
    return KBE_YUV_ABI_VERSION;
}

KBE_YUV_API size_t kbe_yuv420_bytes(int W, int H)
{
    return ky::payload_bytes(W, H);
}

KBE_YUV_API int kbe_yuv420_u8(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, uint8_t* const* out_u8, int flags, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!out_u8) what = "null out_u8";
    else if (n_frames < 1) what = "n_frames < 1";
    else if (!(W >= 1 && W <= ky::kMaxSide && H >= 1 && H <= ky::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (flags & ~KBE_YUV_BGR) what = "unknown bits in flags";
    for (int i = 0; !what && i < n_frames; i++)
        if (!frames_u8[i]) what = "null element of frames_u8";
    for (int i = 0; !what && i < n_frames; i++)
        if (!out_u8[i]) what = "null element of out_u8";
    // a lane reads its frame's bytes and writes the payload's: a payload may share no byte with a source of the call, nor with another payload
    if (!what) {
        const uintptr_t src_bytes = frame_extent(H, stride_bytes, 3u * (uintptr_t) W), out_bytes = (uintptr_t) ky::payload_bytes(W, H);
        if (any_overlap(out_u8, n_frames, out_bytes, frames_u8, n_frames, src_bytes)) what = "an element of out_u8 overlaps a source frame";
        else if (any_two_overlap(out_u8, n_frames, out_bytes)) what = "an element of out_u8 overlaps another output";
    }
    if (what) return refuse("kbe_yuv420_u8", what);

    YuvArgs a;
    a.k = ky::coef(flags);
    a.W = (uint32_t) W;
    a.H = (uint32_t) H;
    a.stride = (uint32_t) stride_bytes;
    const unsigned pairs = blocks_for((size_t) ((H + 1) / 2), kRowPairs);
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = launch_frames(n_frames, f0, kFramesPerLaunch);
        fill_slots(a.src, frames_u8, f0, nf);
        fill_slots(a.dst, out_u8, f0, nf);
        hipLaunchKernelGGL(k_yuv420, dim3(pairs, 1, (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_yuv420_u8");
}

}  // extern "C"
