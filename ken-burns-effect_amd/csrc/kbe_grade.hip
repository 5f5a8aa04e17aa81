// kbe_grade.hip -- kbe_grade_u8: a 3D lookup table with tetrahedral interpolation applied to frames that lie in HBM, in place, for grade.py
// (include/kbe_grade.h).  The arithmetic is kbe_grade_block.h's grade_run(), run_from_aligned() and run_to_aligned(), as they are; this
// file spreads the work over the chip.  Unlike the other frame filters, which stream or gather from neighbouring pixels, this one makes
// data-dependent gathers: four table nodes per pixel, anywhere in the table.
//
// The table lives in LDS.  A workgroup first copies its N^3 dwords there -- 16 bytes per lane and step at the table's dword alignment,
// coalesced, stored 16 bytes wide --, waits once, and then gathers four dwords per pixel from it.  The copy is paid once per workgroup, so a
// workgroup takes many ITEMS through a loop whose bound, the trips, the host works out: an item is one wave's share, kSpanPixels = 1024
// pixels of one row of one frame, and item (trip * gridDim.x + blockIdx.x) * waves + wave is the wave's in that trip.  The grid is sized by
// the work and capped by what the 256 CUs hold at the table's LDS size.  The LDS is static and comes in four sizes, for tables of up to 9,
// 17, 25 and 33 nodes per axis (2 916, 19 652, 62 500 and 143 748 bytes): a CU holds eight workgroups of 256 threads of the first two, two of
// 512 threads of the third and one of 1024 threads of the last -- gfx950's 160 KiB of LDS per CU are what lets a 33-point table fit at all.
//
// In place: an output byte depends on all three bytes of its pixel, so no lane may read a byte that another lane writes.  Ownership is by
// whole pixels: a lane takes a RUN of 16 pixels, 48 bytes of a row, and loads and stores exactly those bytes.  48 is a multiple of 16: every
// run of a row has the alignment of the row's first byte.  On a multiple of 16 the run is three 16-byte pieces; on a multiple of 4 the same
// at a dword's alignment; elsewhere the 1..3 bytes up to the next dword and those behind the last whole one go byte by byte and the eleven
// aligned dwords between them as 16 + 16 + 12 bytes.  A row's last run, when it is shorter than 16 pixels, goes byte by byte.  Nothing
// outside a row's 3 W bytes is read or written.
//
// The pointers and every frame's strength travel as kernel arguments: a launch carries kFramesPerLaunch = 12 frames.  Every loop has a
// static bound (the table's size, the trips); the only wait is the workgroup's own, behind the copy; no workgroup waits for another; no scratch.
#include "kbe_grade.h"
#include "kbe_grade_block.h"
#include "kbe_host.h"

using namespace kbe;
namespace kgr = kbe_grade;

namespace {

constexpr int kFramesPerLaunch = KBE_GRADE_FRAMES_PER_LAUNCH;
constexpr int kLanes = 64;
constexpr int kSpanPixels = kLanes * kgr::kRunPixels;       // 1024: the pixels of a row that one wave takes in one trip
constexpr int kCUs = 256;                                   // of the MI355X: what caps the grid
static_assert(kSpanPixels == 1024 && kFramesPerLaunch == kbe_rows::kFramesPerLaunch && kgr::kRunBytes == 48, "the kernel's layout");

using kbe_rows::Dwords3;
using kbe_rows::Dwords4;

struct GradeArgs {
    uint8_t* frame[kFramesPerLaunch];
    uint32_t strength[kFramesPerLaunch];                    // 1..256
    const uint32_t* lut;
    uint32_t N, W, stride, segments, per_frame, items, trips;      // segments: the spans of a row; per_frame = H * segments; items = frames * per_frame
};

template <int kNodes, int kThreads>
__global__ __launch_bounds__(kThreads) void k_grade(const GradeArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t table[kNodes * kNodes * kNodes];
    constexpr uint32_t kWaves = kThreads / kLanes;
    {
        const uint32_t dwords = a.N * a.N * a.N, whole = dwords & ~3u;
        for (uint32_t at = 4u * threadIdx.x; at < whole; at += 4u * kThreads) {
            const Dwords4 four = *reinterpret_cast<const Dwords4*>(a.lut + at);
            *reinterpret_cast<uint4*>(table + at) = make_uint4(four.x, four.y, four.z, four.w);
        }
        if (threadIdx.x < dwords - whole) table[whole + threadIdx.x] = a.lut[whole + threadIdx.x];
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & (kLanes - 1), wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x / kLanes));
    for (uint32_t trip = 0; trip < a.trips; trip++) {
        const uint32_t item = (trip * gridDim.x + blockIdx.x) * kWaves + wave;
        if (item >= a.items) break;                                                                   // (the items only grow with the trips)
        const uint32_t f = item / a.per_frame, rest = item - f * a.per_frame, y = rest / a.segments, segment = rest - y * a.segments;
        const uint32_t first = segment * kSpanPixels + kgr::kRunPixels * lane;                        // this lane takes the pixels [first, first + count)
        if (first >= a.W) continue;
        const uint32_t count = a.W - first < (uint32_t) kgr::kRunPixels ? a.W - first : (uint32_t) kgr::kRunPixels, s = a.strength[f];
        uint8_t* const p = a.frame[f] + (size_t) y * a.stride + 3u * (size_t) first;
        const uint32_t b = (uint32_t) ((uintptr_t) p & 3u);
        uint32_t c[kgr::kRunDwords], x[kgr::kRunDwords + 1];
        const bool whole = count == (uint32_t) kgr::kRunPixels, on16 = ((uintptr_t) p & 15u) == 0u;
        uint8_t* const base = p - b;                                                                  // (used where b != 0: the aligned dword in which the run begins)
        if (!whole) {
            // a row's last run: its 3 * count bytes, one by one
            for (int d = 0; d < kgr::kRunDwords; d++) {
                c[d] = 0u;
                for (int k = 0; k < 4; k++)
                    if ((uint32_t) (4 * d + k) < 3u * count) c[d] |= (uint32_t) p[4 * d + k] << (8 * k);
            }
        } else if (on16) {
            const uint4* const q = reinterpret_cast<const uint4*>(p);
            const uint4 m0 = q[0], m1 = q[1], m2 = q[2];
            c[0] = m0.x, c[1] = m0.y, c[2] = m0.z, c[3] = m0.w, c[4] = m1.x, c[5] = m1.y, c[6] = m1.z, c[7] = m1.w, c[8] = m2.x, c[9] = m2.y, c[10] = m2.z, c[11] = m2.w;
        } else if (b == 0u) {
            const Dwords4* const q = reinterpret_cast<const Dwords4*>(p);
            const Dwords4 m0 = q[0], m1 = q[1], m2 = q[2];
            c[0] = m0.x, c[1] = m0.y, c[2] = m0.z, c[3] = m0.w, c[4] = m1.x, c[5] = m1.y, c[6] = m1.z, c[7] = m1.w, c[8] = m2.x, c[9] = m2.y, c[10] = m2.z, c[11] = m2.w;
        } else {
            // the run's bytes are the bytes [b, b + 48) of 13 aligned dwords: of the first and the last only the run's own bytes are touched
            x[0] = 0u;
            x[kgr::kRunDwords] = (uint32_t) base[kgr::kRunBytes];
            for (uint32_t k = 1; k < 4u; k++) {
                if (k >= b) x[0] |= (uint32_t) base[k] << (8u * k);
                if (k < b) x[kgr::kRunDwords] |= (uint32_t) base[kgr::kRunBytes + k] << (8u * k);
            }
            const Dwords4 m0 = *reinterpret_cast<const Dwords4*>(base + 4), m1 = *reinterpret_cast<const Dwords4*>(base + 20);
            const Dwords3 m2 = *reinterpret_cast<const Dwords3*>(base + 36);
            x[1] = m0.x, x[2] = m0.y, x[3] = m0.z, x[4] = m0.w, x[5] = m1.x, x[6] = m1.y, x[7] = m1.z, x[8] = m1.w, x[9] = m2.x, x[10] = m2.y, x[11] = m2.z;
            kgr::run_from_aligned(x, b, c);
        }

        kgr::grade_run(c, table, a.N, s);

        if (!whole) {
            for (int d = 0; d < kgr::kRunDwords; d++)
                for (int k = 0; k < 4; k++)
                    if ((uint32_t) (4 * d + k) < 3u * count) p[4 * d + k] = (uint8_t) (c[d] >> (8 * k));
        } else if (on16) {
            uint4* const q = reinterpret_cast<uint4*>(p);
            q[0] = make_uint4(c[0], c[1], c[2], c[3]), q[1] = make_uint4(c[4], c[5], c[6], c[7]), q[2] = make_uint4(c[8], c[9], c[10], c[11]);
        } else if (b == 0u) {
            Dwords4* const q = reinterpret_cast<Dwords4*>(p);
            q[0] = Dwords4{c[0], c[1], c[2], c[3]}, q[1] = Dwords4{c[4], c[5], c[6], c[7]}, q[2] = Dwords4{c[8], c[9], c[10], c[11]};
        } else {
            kgr::run_to_aligned(c, b, x);
            base[kgr::kRunBytes] = (uint8_t) x[kgr::kRunDwords];
            for (uint32_t k = 1; k < 4u; k++) {
                if (k >= b) base[k] = (uint8_t) (x[0] >> (8u * k));
                if (k < b) base[kgr::kRunBytes + k] = (uint8_t) (x[kgr::kRunDwords] >> (8u * k));
            }
            *reinterpret_cast<Dwords4*>(base + 4) = Dwords4{x[1], x[2], x[3], x[4]};
            *reinterpret_cast<Dwords4*>(base + 20) = Dwords4{x[5], x[6], x[7], x[8]};
            *reinterpret_cast<Dwords3*>(base + 36) = Dwords3{x[9], x[10], x[11]};
        }
    }
}

// One launch of the kernel whose LDS holds kNodes^3 dwords, with workgroups of kThreads of which a CU holds kPerCU
template <int kNodes, int kThreads, int kPerCU>
void launch_class(GradeArgs& a, hipStream_t stream)
{
    const uint32_t groups = blocks_for((size_t) a.items, kThreads / kLanes), most = (uint32_t) (kCUs * kPerCU), grid = groups < most ? groups : most;
    a.trips = (groups + grid - 1u) / grid;
    hipLaunchKernelGGL((k_grade<kNodes, kThreads>), dim3(grid), dim3(kThreads), 0, stream, a);
}

}  // namespace

extern "C" {

KBE_GRADE_API int kbe_grade_abi_version(void)
{
    return KBE_GRADE_ABI_VERSION;
}

KBE_GRADE_API int kbe_grade_u8(uint8_t* const* frames_u8, int n, int W, int H, int stride_bytes, const uint32_t* lut, int N, const int32_t* strength,
                               kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!frames_u8) what = "null frames_u8";
    else if (!lut) what = "null lut";
    else if (!strength) what = "null strength";
    else if (n < 1) what = "n < 1";
    else if (!(W >= 1 && W <= kgr::kMaxSide && H >= 1 && H <= kgr::kMaxSide)) what = "W or H outside 1..65535";
    else if (stride_bytes < 3 * W) what = "stride_bytes < 3 W";
    else if (!(N >= kgr::kMinNodes && N <= kgr::kMaxNodes)) what = "N outside 2..33";
    else if ((uintptr_t) lut & 3u) what = "lut is not 4-byte aligned";
    for (int i = 0; !what && i < n; i++) {
        if (!frames_u8[i]) what = "null element of frames_u8";
        else if (!(strength[i] >= 0 && strength[i] <= kgr::kMaxStrength)) what = "an element of strength outside 0..256";
    }
    // a lane reads and writes its frame's bytes and the workgroups read the table's: a frame may share no byte with another frame of the call, nor with the table
    if (!what) {
        const uintptr_t frame_bytes = frame_extent(H, stride_bytes, 3u * (uintptr_t) W);
        if (any_overlap(frames_u8, n, frame_bytes, &lut, 1, 4u * (uintptr_t) (N * N * N))) what = "an element of frames_u8 overlaps the table";
        else if (any_two_overlap(frames_u8, n, frame_bytes)) what = "an element of frames_u8 overlaps another frame";
    }
    if (what) return refuse("kbe_grade_u8", what);

    GradeArgs a;
    a.lut = lut;
    a.N = (uint32_t) N, a.W = (uint32_t) W, a.stride = (uint32_t) stride_bytes;
    a.segments = blocks_for((size_t) W, kSpanPixels);
    a.per_frame = (uint32_t) H * a.segments;                                     // at most 65535 * 64
    int held = 0;
    const auto launch = [&]() {
        for (int i = held; i < kFramesPerLaunch; i++) a.frame[i] = nullptr, a.strength[i] = 0u;
        a.items = (uint32_t) held * a.per_frame;                                 // at most 12 * 65535 * 64 < 2^26
        if (N <= 9) launch_class<9, 256, 8>(a, (hipStream_t) stream);
        else if (N <= 17) launch_class<17, 256, 8>(a, (hipStream_t) stream);
        else if (N <= 25) launch_class<25, 512, 2>(a, (hipStream_t) stream);
        else launch_class<33, 1024, 1>(a, (hipStream_t) stream);
        held = 0;
    };
    for (int i = 0; i < n; i++) {
        if (strength[i] == 0) continue;                                          // in no launch
        a.frame[held] = frames_u8[i], a.strength[held] = (uint32_t) strength[i];
        if (++held == kFramesPerLaunch) launch();
    }
    if (held) launch();
    return launched("kbe_grade_u8");
}

}  // extern "C"
