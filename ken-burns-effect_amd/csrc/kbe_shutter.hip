// kbe_shutter.hip -- kbe_shutter_mean_u8: every output frame the byte-wise mean of `samples` source frames that lie in HBM, for shutter.py
// (include/kbe_shutter.h).  The arithmetic is kbe_shutter_block.h's add() and finish(), as they are, and the rows' bytes are taken and
// stored by kbe_rows.h's realign() and store_piece(), which k_transition runs too; this file spreads the work over the chip.
// A streaming kernel: it reads S * 3 W H bytes and writes 3 W H per output, and nothing is read twice.
//
// A row is a byte stream.  One lane makes one ALIGNED 16-byte piece of an output row; a wave takes kSpan = 1024 bytes of one row, counted from
// the row's address rounded down to 16, and the four waves of a workgroup take four rows.  For every source the lane's 16 bytes start at the
// source row's own alignment, b = 0..3 bytes into an aligned dword: the lane loads the five aligned dwords that hold them -- the first four
// as one 16-byte piece at a dword's alignment, which the chip's global loads take, and the fifth on its own; at a row's two ends dword by
// dword, and only the dwords that hold a byte of the row: no address outside a row's dwords is touched -- and cuts its 16 bytes out with a
// funnel shift by bytes.  No register is indexed by a variable.  Neighbouring lanes load each other's fifth dword: that costs L1 bandwidth,
// not HBM traffic.  The sums are two 16-bit lanes per dword.  A piece that lies inside the row is stored as 16 bytes; the pieces at a row's
// two ends as dwords and single bytes (kbe_rows.h's store_piece, the tile kernels' too); nothing outside a row's 3 W bytes is written.
//
// The pointer tables travel as kernel arguments: a launch carries min(12, max(1, 96 / S)) output frames (the grid's z), so at most 96 source
// pointers.  Every loop has a static bound (the S sources); no workgroup waits for another; no LDS, no scratch.
#include "kbe_shutter.h"
#include "kbe_shutter_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace ksh = kbe_shutter;

namespace {

constexpr int kOutputsPerLaunch = kbe_rows::kFramesPerLaunch;
constexpr int kSourcesPerLaunch = 96;
constexpr int kRows = 4;                                    // one wave per row
constexpr int kLanes = 64;
constexpr int kSpan = kLanes * ksh::kPiece;                 // 1024: the bytes of a row that one workgroup takes
static_assert(kRows * kLanes == kBlock && kSpan == 1024 && kOutputsPerLaunch * 8 == kSourcesPerLaunch, "the kernel's layout");

using kbe_rows::Dwords4;

struct ShutterArgs {
    const uint8_t* src[kSourcesPerLaunch];                  // the sources of output i: src[i * S .. i * S + S - 1]
    uint8_t* dst[kOutputsPerLaunch];
    uint32_t S, M;                                          // M = magic(S)
    uint32_t row_bytes, H, stride, out_stride;
};

__host__ __device__ constexpr int outputs_per_launch(int S)
{
    return kSourcesPerLaunch / S < 1 ? 1 : (kSourcesPerLaunch / S > kOutputsPerLaunch ? kOutputsPerLaunch : kSourcesPerLaunch / S);
}

__global__ __launch_bounds__(kBlock) void k_shutter_mean(const ShutterArgs a)
{
    const uint32_t lane = threadIdx.x & (kLanes - 1), y = blockIdx.y * kRows + threadIdx.x / kLanes;
    if (y >= a.H) return;
    uint8_t* const row = a.dst[blockIdx.z] + (size_t) y * a.out_stride;
    const uint32_t lead = (uint32_t) ((uintptr_t) row & 15u), end = lead + a.row_bytes;       // the row's bytes are [lead, end) of its pieces
    const uint32_t at = blockIdx.x * kSpan + ksh::kPiece * lane;                              // this lane takes the piece [at, at + 16)
    if (at >= end) return;
    const long j0 = (long) at - (long) lead, row_bytes = (long) a.row_bytes;                  // the piece's first byte, as a byte of the row

    ksh::Acc acc;
    ksh::clear(acc);
    const uint32_t S = a.S;
    const uint8_t* const* const sources = a.src + blockIdx.z * S;
    const size_t row_at = (size_t) y * a.stride;
    // (inside the row, which is all but a row's first and last piece or two, every dword holds a byte of it.  One source at a time: taking
    // turns with it on the chip, four sources in flight per wave and the fifth dword fetched from the next lane's registers were both slower)
    const bool inside = kbe_rows::all_dwords_hold_a_byte<ksh::kDwords>(j0, row_bytes);
    for (uint32_t s = 0; s < S; s++) {
        const uint8_t* const first = sources[s] + row_at + j0;                                // (before the row where j0 < 0: not read)
        const uint32_t b = (uint32_t) ((uintptr_t) first & 3u);
        const uint32_t* const dwords = reinterpret_cast<const uint32_t*>(first - b);
        uint32_t x[5], w[4];
        if (inside) {
            const Dwords4 four = *reinterpret_cast<const Dwords4*>(dwords);
            x[0] = four.x, x[1] = four.y, x[2] = four.z, x[3] = four.w, x[4] = dwords[4];
        } else {
            for (int k = 0; k < 5; k++) x[k] = kbe_rows::dword_holds_a_byte<ksh::kDwords>(j0, b, k, row_bytes) ? dwords[k] : 0u;
        }
        ksh::realign(x, b, w);
        ksh::add(acc, w);
    }
    uint32_t word[4];
    ksh::finish(acc, S, a.M, word);
    kbe_rows::store_piece(row, lead, end, at, word);
}

}  // namespace

extern "C" {

KBE_SHUTTER_API int kbe_shutter_abi_version(void)
{
    return KBE_SHUTTER_ABI_VERSION;
}

KBE_SHUTTER_API int kbe_shutter_mean_u8(const uint8_t* const* frames_u8, int n_out, int samples, int W, int H, int stride_bytes, uint8_t* const* out_u8,
                                        int out_stride_bytes, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!out_u8) what = "null out_u8";
    else if (n_out < 1) what = "n_out < 1";
    else if (!(samples >= 1 && samples <= ksh::kMaxSamples)) what = "samples outside 1..32";
    else if (!(W >= 1 && W <= ksh::kMaxSide && H >= 1 && H <= ksh::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (out_stride_bytes < 3 * W) what = "out_stride_bytes < 3 W";
    const size_t n_sources = what ? 0u : (size_t) n_out * (size_t) samples;
    for (size_t i = 0; !what && i < n_sources; i++)
        if (!frames_u8[i]) what = "null element of frames_u8";
    for (int i = 0; !what && i < n_out; i++)
        if (!out_u8[i]) what = "null element of out_u8";
    // a lane reads its sources' bytes and writes the output's: an output may share no byte with a source of the call, nor with another output
    if (!what) {
        const uintptr_t src_bytes = frame_extent(H, stride_bytes, 3u * (uintptr_t) W), out_bytes = frame_extent(H, out_stride_bytes, 3u * (uintptr_t) W);
        if (any_overlap(out_u8, n_out, out_bytes, frames_u8, n_sources, src_bytes)) what = "an element of out_u8 overlaps a source frame";
        else if (any_two_overlap(out_u8, n_out, out_bytes)) what = "an element of out_u8 overlaps another output";
    }
    if (what) return refuse("kbe_shutter_mean_u8", what);

    ShutterArgs a;
    a.S = (uint32_t) samples;
    a.M = ksh::magic(a.S);
    a.row_bytes = 3u * (uint32_t) W;
    a.H = (uint32_t) H;
    a.stride = (uint32_t) stride_bytes;
    a.out_stride = (uint32_t) out_stride_bytes;
    const int per_launch = outputs_per_launch(samples);
    // (a row's pieces begin up to 15 bytes before the row does)
    const dim3 spans(blocks_for((size_t) a.row_bytes + 15u, kSpan), blocks_for((size_t) H, kRows));
    for (int f0 = 0; f0 < n_out; f0 += per_launch) {
        const int nf = launch_frames(n_out, f0, per_launch);
        fill_slots(a.src, frames_u8, (size_t) f0 * samples, nf * samples);
        fill_slots(a.dst, out_u8, f0, nf);
        hipLaunchKernelGGL(k_shutter_mean, dim3(spans.x, spans.y, (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_shutter_mean_u8");
}

}  // extern "C"
