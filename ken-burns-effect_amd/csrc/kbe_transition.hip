// kbe_transition.hip -- kbe_transition_u8: every output frame made of two source frames that lie in HBM -- a dissolve, a wipe with a soft edge, a
// fade through a colour --, for transition.py (include/kbe_transition.h).  The arithmetic is kbe_transition_block.h's plan() and blend_piece()
// and kbe_rows.h's realign() and store_piece(), as they are; this file spreads the work over the chip.  A streaming kernel in the shape of
// k_shutter_mean (kbe_shutter.hip): it reads up to 2 * 3 W H bytes and writes 3 W H per output, and nothing is read twice.
//
// A row is a byte stream.  One lane makes one ALIGNED 16-byte piece of an output row; a wave takes kSpan = 1024 bytes of one row, counted from
// the row's address rounded down to 16, and the four waves of a workgroup take four rows.  For each source the lane's 16 bytes start at the
// source row's own alignment, b = 0..3 bytes into an aligned dword: the lane loads the five aligned dwords that hold them -- the first four
// as one 16-byte piece at a dword's alignment, the fifth on its own; at a row's two ends dword by dword, and only the dwords that hold a
// byte of the row -- and cuts its 16 bytes out with a funnel shift by bytes; both sources' dwords are loaded before either is cut, so the two
// loads are in flight together.  A lane asks plan() first which sources its piece reads: a piece
// of a wipe outside the soft edge is a copy of one source, the fade blends one source with the colour, and the other source is not loaded.
// A piece that lies inside the row is stored as 16 bytes; the pieces at a row's two ends as dwords and single bytes; nothing outside a
// row's 3 W bytes is written.
//
// The pointer tables and the frames' progress travel as kernel arguments: a launch carries kFramesPerLaunch = 12 output frames (the grid's
// z).  Every loop has a static bound; no workgroup waits for another; no LDS, no scratch.
#include "kbe_transition.h"
#include "kbe_transition_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace ktr = kbe_transition;

namespace {

constexpr int kFramesPerLaunch = KBE_TRANSITION_FRAMES_PER_LAUNCH;
constexpr int kRows = 4;                                    // one wave per row
constexpr int kLanes = 64;
constexpr int kSpan = kLanes * ktr::kPiece;                 // 1024: the bytes of a row that one workgroup takes
static_assert(kRows * kLanes == kBlock && kSpan == 1024 && kFramesPerLaunch == kbe_rows::kFramesPerLaunch, "the kernel's layout");

using kbe_rows::Dwords4;

struct TransitionArgs {
    const uint8_t* from[kFramesPerLaunch];
    const uint8_t* to[kFramesPerLaunch];
    uint8_t* dst[kFramesPerLaunch];
    uint32_t progress[kFramesPerLaunch];
    ktr::Frame frame;                                       // (its p: per output, from progress)
    uint32_t row_bytes, stride, out_stride;
};

// the five aligned dwords around the 16 bytes of a source row that start at `first`, the byte j0 of the row, b bytes into the first of them.
// Loading and cutting are two steps, so that the loads of both sources are in flight before the first of them is waited for
__device__ __forceinline__ uint32_t load_dwords(const uint8_t* first, long j0, long row_bytes, bool inside, uint32_t x[5])
{
    const uint32_t b = (uint32_t) ((uintptr_t) first & 3u);
    const uint32_t* const dwords = reinterpret_cast<const uint32_t*>(first - b);
    if (inside) {
        const Dwords4 four = *reinterpret_cast<const Dwords4*>(dwords);
        x[0] = four.x, x[1] = four.y, x[2] = four.z, x[3] = four.w, x[4] = dwords[4];
    } else {
        for (int k = 0; k < 5; k++) x[k] = kbe_rows::dword_holds_a_byte<ktr::kDwords>(j0, b, k, row_bytes) ? dwords[k] : 0u;
    }
    return b;
}

__global__ __launch_bounds__(kBlock) void k_transition(const TransitionArgs a)
{
    const uint32_t lane = threadIdx.x & (kLanes - 1), y = blockIdx.y * kRows + threadIdx.x / kLanes;
    if (y >= a.frame.H) return;
    uint8_t* const row = a.dst[blockIdx.z] + (size_t) y * a.out_stride;
    const uint32_t lead = (uint32_t) ((uintptr_t) row & 15u), end = lead + a.row_bytes;       // the row's bytes are [lead, end) of its pieces
    const uint32_t at = blockIdx.x * kSpan + ktr::kPiece * lane;                              // this lane takes the piece [at, at + 16)
    if (at >= end) return;
    const long j0 = (long) at - (long) lead, row_bytes = (long) a.row_bytes;                  // the piece's first byte, as a byte of the row

    ktr::Frame f = a.frame;
    f.p = a.progress[blockIdx.z];
    const ktr::Plan q = ktr::plan(f, j0, y);
    const size_t row_at = (size_t) y * a.stride;
    const bool inside = kbe_rows::all_dwords_hold_a_byte<ktr::kDwords>(j0, row_bytes);
    uint32_t xf[5] = {0u, 0u, 0u, 0u, 0u}, xt[5] = {0u, 0u, 0u, 0u, 0u}, bf = 0u, bt = 0u, from[4], to[4], word[4];
    // (before the row where j0 < 0: not read)
    if (q.from) bf = load_dwords(a.from[blockIdx.z] + row_at + j0, j0, row_bytes, inside, xf);
    if (q.to) bt = load_dwords(a.to[blockIdx.z] + row_at + j0, j0, row_bytes, inside, xt);
    ktr::realign(xf, bf, from);
    ktr::realign(xt, bt, to);
    ktr::blend_piece(f, q, from, to, word);
    kbe_rows::store_piece(row, lead, end, at, word);
}

}  // namespace

extern "C" {

KBE_TRANSITION_API int kbe_transition_abi_version(void)
{
    return KBE_TRANSITION_ABI_VERSION;
}

KBE_TRANSITION_API int kbe_transition_u8(const uint8_t* const* from_u8, const uint8_t* const* to_u8, int n, int W, int H, int stride_bytes, int kind,
                                         const int32_t* progress, int softness, uint32_t colour, uint8_t* const* out_u8, int out_stride_bytes,
                                         kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!from_u8) what = "null from_u8";
    else if (!to_u8) what = "null to_u8";
    else if (!out_u8) what = "null out_u8";
    else if (!progress) what = "null progress";
    else if (n < 1) what = "n < 1";
    else if (!(W >= 1 && W <= ktr::kMaxSide && H >= 1 && H <= ktr::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (out_stride_bytes < 3 * W) what = "out_stride_bytes < 3 W";
    else if (!(kind >= 0 && kind < ktr::kKinds)) what = "kind outside 0..5";
    else if (!(softness >= 1 && softness <= ktr::kMaxSoftness)) what = "softness outside 1..65535";
    else if (colour >> 24) what = "colour with bits 24..31 set";
    for (int i = 0; !what && i < n; i++) {
        if (!from_u8[i]) what = "null element of from_u8";
        else if (!to_u8[i]) what = "null element of to_u8";
        else if (!out_u8[i]) what = "null element of out_u8";
        else if (!(progress[i] >= 0 && progress[i] <= 256)) what = "an element of progress outside 0..256";
    }
    // a lane reads its sources' bytes and writes the output's: an output may share no byte with a source of the call, nor with another output
    if (!what) {
        const uintptr_t src_bytes = frame_extent(H, stride_bytes, 3u * (uintptr_t) W), out_bytes = frame_extent(H, out_stride_bytes, 3u * (uintptr_t) W);
        if (any_overlap(out_u8, n, out_bytes, from_u8, n, src_bytes) || any_overlap(out_u8, n, out_bytes, to_u8, n, src_bytes)) what = "an element of out_u8 overlaps a source frame";
        else if (any_two_overlap(out_u8, n, out_bytes)) what = "an element of out_u8 overlaps another output";
    }
    if (what) return refuse("kbe_transition_u8", what);

    TransitionArgs a;
    a.frame.kind = (uint32_t) kind;
    a.frame.p = 0u;
    a.frame.s = (uint32_t) softness;
    a.frame.colour = colour;
    a.frame.W = (uint32_t) W;
    a.frame.H = (uint32_t) H;
    a.frame.M = ktr::magic(a.frame.s);
    a.row_bytes = 3u * (uint32_t) W;
    a.stride = (uint32_t) stride_bytes;
    a.out_stride = (uint32_t) out_stride_bytes;
    // (a row's pieces begin up to 15 bytes before the row does)
    const dim3 spans(blocks_for((size_t) a.row_bytes + 15u, kSpan), blocks_for((size_t) H, kRows));
    for (int f0 = 0; f0 < n; f0 += kFramesPerLaunch) {
        const int nf = launch_frames(n, f0, kFramesPerLaunch);
        fill_slots(a.from, from_u8, f0, nf);
        fill_slots(a.to, to_u8, f0, nf);
        fill_slots(a.dst, out_u8, f0, nf);
        for (int i = 0; i < kFramesPerLaunch; i++) a.progress[i] = i < nf ? (uint32_t) progress[f0 + i] : 0u;
        hipLaunchKernelGGL(k_transition, dim3(spans.x, spans.y, (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a);
    }
    return launched("kbe_transition_u8");
}

}  // extern "C"
