// kbe_mjpeg.hip -- kbe_mjpeg_encode: frames that lie in HBM as baseline JPEG streams, back to back, for the Motion-JPEG video writers
// (include/kbe.h).  The stream and all of its arithmetic are defined in kbe_mjpeg_block.h; this file spreads that work over the chip.
//
// A frame's restart intervals (kRestartMcus MCUs each) are independent, but where an interval's bytes go depends on the lengths of all
// intervals in front of it.  So the work is done twice, with nothing but 12 bytes per interval in HBM between the two passes:
//   1. k_mjpeg_encode<false>: a workgroup takes kGroupIntervals intervals: samples (colour conversion, chroma average), the 8 x 8 DCTs with
//      eight lanes per block (rows in registers, transpose through LDS, columns), quantisation into LDS; then one lane per BLOCK packs the
//      block's Huffman codes and value bits into words of its own in LDS, and one lane per interval sends them on, in order, into a sink
//      that counts the stream's bytes (stuffed 0xFF, padding, RSTm): the interval's LENGTH is all that is stored;
//   2. an exclusive scan of the lengths over all intervals of all frames of the launch (kbe_units_scan.h: sums of 256, a scan of the sums, apply): every
//      interval's place, every frame's offsets[i], the total and `status`;
//   3. k_mjpeg_encode<true>: the same code again, the sink now storing the bytes at their place (nothing at or beyond `cap`).
// No kernel waits for another workgroup.  n frames are cut into launches of kFramesPerLaunch.
#include "kbe_host.h"
#include "kbe_mjpeg_block.h"
#include "kbe_units_scan.h"

using namespace kbe;
using namespace kbe_mjpeg;

namespace {

constexpr int kGroupIntervals = 4;                                              // intervals per workgroup: one per wave in the entropy phase
constexpr int kGroupBlocks = kGroupIntervals * kRestartMcus * 6;                // 96 blocks
constexpr int kEncodeThreads = 64 * kGroupIntervals;
constexpr int kBlocksAtOnce = kEncodeThreads / 8;                               // eight lanes per block
static_assert(kGroupBlocks % kBlocksAtOnce == 0, "the DCT loop takes whole rounds");

struct EncodeArgs {
    const uint8_t* frames[kFramesPerLaunch];
    Geometry g;
    Tables t;
};
static_assert(sizeof(EncodeArgs) <= 3840, "kernel arguments: 4 KB at most");

struct CountSink {
    uint32_t n;
    __device__ __forceinline__ void put(unsigned) { n++; }
};

// bytes to their place: singly up to the first 4-byte boundary, then four at a time, the rest singly; never at or beyond cap
struct StoreSink {
    uint8_t* base;
    uint64_t pos, cap;
    uint32_t word;
    int k;
    __device__ __forceinline__ void put(unsigned v)
    {
        if (k == 0 && (((uintptr_t) base + pos) & 3u)) {
            if (pos < cap) base[pos] = (uint8_t) v;
            pos++;
            return;
        }
        word |= v << (8 * k);
        if (++k == 4) {
            if (pos + 4 <= cap) *reinterpret_cast<uint32_t*>(base + pos) = word;
            else tail();
            pos += 4;
            word = 0;
            k = 0;
        }
    }
    __device__ __forceinline__ void tail()
    {
        for (int i = 0; i < k; i++)
            if (pos + i < cap) base[pos + i] = (uint8_t) (word >> (8 * i));
    }
    __device__ __forceinline__ void finish() { tail(); pos += k; k = 0; }
};

template <bool STORE>
__global__ __launch_bounds__(kEncodeThreads) void k_mjpeg_encode(const EncodeArgs a, uint32_t* __restrict__ counts, const uint64_t* __restrict__ starts,
                                                                 uint8_t* __restrict__ streams, uint64_t cap)
{
    __shared__ int16_t s_zz[kGroupBlocks * 64];
    // (the DCT's transposes, then the blocks' packed bits: one after the other in the same bytes)
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[kGroupBlocks * kBlockWords];
    __shared__ int s_nbits[kGroupBlocks];
    static_assert(sizeof(s_raw) >= sizeof(float) * kBlocksAtOnce * 8 * 9, "the transposes fit");
    float (*s_tr)[8][9] = reinterpret_cast<float (*)[8][9]>(s_raw);
    __shared__ float s_rq[2][64];
    __shared__ uint32_t s_dc[2][12], s_ac[2][256];
    __shared__ uint8_t s_scan[64];

    const int tid = (int) threadIdx.x, frame = (int) blockIdx.y;
    const Geometry g = a.g;
    const int interval0 = (int) blockIdx.x * kGroupIntervals;
    for (int i = tid; i < 128; i += kEncodeThreads) (&s_rq[0][0])[i] = (&a.t.rq[0][0])[i];
    for (int i = tid; i < 512; i += kEncodeThreads) (&s_ac[0][0])[i] = (&a.t.ac[0][0])[i];
    if (tid < 24) (&s_dc[0][0])[tid] = (&a.t.dc[0][0])[tid];
    if (tid < 64) s_scan[tid] = a.t.scan_of[tid];
    __syncthreads();

    // samples, DCT, quantisation: eight lanes per block, lane r takes row r and then column r
    const uint8_t* src = a.frames[frame];
    const int lane = tid & 7, slot = tid >> 3;
    for (int round = 0; round < kGroupBlocks / kBlocksAtOnce; round++) {
        const int blk = round * kBlocksAtOnce + slot, comp = blk % 6;
        const int mcu = interval0 * kRestartMcus + blk / 6;
        const bool live = mcu < g.mcus;
        float v[8];
        if (live) {
            block_row(src, g, mcu % g.mcus_x, mcu / g.mcus_x, comp, lane, v);
            fdct8(v);
            for (int j = 0; j < 8; j++) s_tr[slot][lane][j] = v[j];
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < 8; i++) v[i] = s_tr[slot][i][lane];
            block_column(v, lane, s_rq[comp < 4 ? 0 : 1], s_scan, s_zz + blk * 64);
        }
        __syncthreads();
    }

    // entropy coding, step 1: one lane per block packs the block's bits into words of its own (a block's bits depend on its coefficients
    // and the DC value in front of it, nothing else)
    if (tid < kGroupBlocks) {
        const int k = tid / (kRestartMcus * 6), within = tid % (kRestartMcus * 6), comp = within % 6;
        const int interval = interval0 + k;
        if (interval < g.intervals && within < interval_mcus(g, interval) * 6) {
            PackedBits packed = { s_raw + tid * kBlockWords, 0, 0, 0 };
            const int16_t* zz = s_zz + k * kRestartMcus * 6 * 64;
            encode_block(packed, zz + within * 64, s_dc[comp < 4 ? 0 : 1], s_ac[comp < 4 ? 0 : 1], dc_predictor(zz, within / 6, comp), nullptr);
            s_nbits[tid] = packed.finish();
        }
    }
    __syncthreads();

    // step 2: an interval's bytes are a serial chain (stuffing, the stream's byte boundaries): lane 0 of wave k sends the bits of interval
    // k's blocks on, in order, into a sink that counts or stores
    const size_t first = (size_t) frame * (size_t) g.intervals;
    if ((tid & 63) == 0) {
        const int k = tid >> 6, interval = interval0 + k;
        if (interval < g.intervals) {
            const int blocks = interval_mcus(g, interval) * 6, blk0 = k * kRestartMcus * 6;
            const uint32_t lead = interval == 0 ? (uint32_t) kHeaderBytes : 0u;        // a frame's header lies in front of its first interval
            if (!STORE) {
                CountSink sink = { 0u };
                StreamBits<CountSink> out = { { 0u, 0 }, sink, nullptr };
                for (int blk = 0; blk < blocks; blk++) replay_bits(out, s_raw + (blk0 + blk) * kBlockWords, s_nbits[blk0 + blk]);
                end_interval(out.b, sink, g, interval, nullptr);
                counts[first + interval] = sink.n + lead;
            } else {
                StoreSink sink = { streams, starts[first + interval] + lead, cap, 0u, 0 };
                StreamBits<StoreSink> out = { { 0u, 0 }, sink, nullptr };
                for (int blk = 0; blk < blocks; blk++) replay_bits(out, s_raw + (blk0 + blk) * kBlockWords, s_nbits[blk0 + blk]);
                end_interval(out.b, sink, g, interval, nullptr);
                sink.finish();
            }
        }
    }
    if (STORE && interval0 == 0) {
        const uint64_t at = starts[first];
        for (int b = tid; b < kHeaderBytes; b += kEncodeThreads)
            if (at + b < cap) streams[at + b] = a.t.header[b];
    }
}

}  // namespace

extern "C" {

size_t kbe_mjpeg_bound(int W, int H)
{
    return W > 0 && H > 0 && W <= 65535 && H <= 65535 ? stream_bound(W, H) : 0;
}

size_t kbe_mjpeg_scratch_bytes(int W, int H, int n_frames)
{
    return W > 0 && H > 0 && W <= 65535 && H <= 65535 && n_frames > 0 ? units_layout((size_t) geometry(W, H, 0, 0).intervals, n_frames, 0).bytes : 0;
}

int kbe_mjpeg_encode(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int quality, int flags, void* scratch, uint8_t* streams, size_t cap,
                     uint64_t* offsets, int* status, kbe_stream_t stream)
{
    const UnitsCall c = { "kbe_mjpeg_encode", frames_u8, n_frames, W, H, scratch, streams, cap, offsets, status, (hipStream_t) stream };
    const int rc = units_check(c, [&]() -> const char* {
        return stride_bytes >= 3 * W && quality >= 1 && quality <= 100 && (flags & ~KBE_MJPEG_BGR) == 0 ? nullptr : "bad stride, quality or flags";
    });
    if (rc != KBE_OK) return rc;

    EncodeArgs a;
    a.g = geometry(W, H, stride_bytes, flags);
    host::tables_build(W, H, quality, &a.t, kRestartMcus);
    return units_encode(c, a, a.g.intervals, 0, [&](bool store, int, int nf, uint32_t* counts, const uint64_t* starts, uint32_t*) {
        const dim3 grid((unsigned) ((a.g.intervals + kGroupIntervals - 1) / kGroupIntervals), (unsigned) nf);
        if (!store) hipLaunchKernelGGL(k_mjpeg_encode<false>, grid, dim3(kEncodeThreads), 0, c.s, a, counts, starts, streams, (uint64_t) cap);
        else hipLaunchKernelGGL(k_mjpeg_encode<true>, grid, dim3(kEncodeThreads), 0, c.s, a, counts, starts, streams, (uint64_t) cap);
    });
}

}  // extern "C"
