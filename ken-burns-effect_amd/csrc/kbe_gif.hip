// kbe_gif.hip -- kbe_gif_encode, kbe_gif_histogram, kbe_gif_lut: frames that lie in HBM as the units of an animated GIF, back to back, for
// gif.py (include/kbe_gif.h).  The unit and all of its arithmetic are defined in kbe_gif_block.h; this file spreads that work over the chip.
//
// A frame's segments (kSegmentPixels indices each) are independent, but where a segment's bytes go depends on the lengths of all segments
// in front of it.  So the work is done twice, with nothing but 12 bytes per segment in HBM between the two passes:
//   1. k_gif_encode<false>: ONE WAVE takes one segment: all lanes fetch its pixels (swap, dither, the table look-up) into LDS and empty
//      the dictionary, an open-addressing table of kHashSlots words in LDS; ONE lane runs the match loop (the header's, as it is) and
//      keeps nothing but the number of codes: the segment's LENGTH is then the header's closed form;
//   2. the exclusive scan of the lengths over all segments of all frames of the launch (kbe_units_scan.h);
//   3. k_gif_encode<true>: the same again with the codes kept in LDS as 16-bit values; all lanes place them at their closed-form bit
//      positions with OR-merges into LDS words, and copy the bytes, sub-block lengths and all, to their place in HBM with plain vector
//      stores (nothing at or beyond `cap`).  The frame's first segment also writes the unit's 19 leading bytes, its last the terminator.
// The serial match loop is this encoder's "one lane per unit" part, as the join of kbe_mjpeg.hip and the code construction of
// kbe_png.hip are.  Every loop has a static bound (the segment's length, the table's size); no kernel waits for another workgroup.
#include "kbe_gif.h"
#include "kbe_gif_block.h"
#include "kbe_host.h"
#include "kbe_units_scan.h"

using namespace kbe;
using namespace kbe_gif;

namespace {

constexpr int kDataWords = (9 + 12 * (kSegmentPixels + 1) + 63 + 31) / 32 + 1;          // a segment's bits, and the word put_bits may touch behind them

struct EncodeArgs {
    const uint8_t* frames[kFramesPerLaunch];
    Geometry g;
    const uint8_t* lut;
    uint8_t lead[kLeadBytes + 1];
};

struct LdsWords {
    uint32_t* w;
    __device__ __forceinline__ void merge(uint32_t index, uint32_t value) { atomicOr(&w[index], value); }
};

struct LdsData {
    const uint32_t* w;
    __device__ __forceinline__ unsigned operator()(uint32_t i) const { return (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu; }
};

// the n framed bytes of a segment's data to out[pos ...), by the whole wave, StoreSink's rule (kbe_mjpeg.hip): singly up to the first 4-byte
// boundary, then four at a time, the rest singly; never at or beyond cap
__device__ __forceinline__ void store_framed(uint8_t* out, uint64_t pos, uint64_t cap, const LdsData& data, uint32_t data_bytes, uint32_t n)
{
    const uint32_t tid = threadIdx.x;
    uint32_t head = (4u - (uint32_t) (((uintptr_t) out + pos) & 3u)) & 3u;
    if (head > n) head = n;
    if (tid < head && pos + tid < cap) out[pos + tid] = (uint8_t) framed_byte(data, data_bytes, tid);
    const uint32_t words = (n - head) / 4u;
    for (uint32_t j = tid; j < words; j += kWave) {
        const uint32_t at = head + 4u * j;
        const uint64_t p = pos + at;
        const uint32_t b0 = framed_byte(data, data_bytes, at), b1 = framed_byte(data, data_bytes, at + 1), b2 = framed_byte(data, data_bytes, at + 2),
                       b3 = framed_byte(data, data_bytes, at + 3);
        if (p + 4 <= cap) *reinterpret_cast<uint32_t*>(out + p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        else {
            if (p < cap) out[p] = (uint8_t) b0;
            if (p + 1 < cap) out[p + 1] = (uint8_t) b1;
            if (p + 2 < cap) out[p + 2] = (uint8_t) b2;
            if (p + 3 < cap) out[p + 3] = (uint8_t) b3;
        }
    }
    for (uint32_t i = head + 4u * words + tid; i < n; i += kWave)
        if (pos + i < cap) out[pos + i] = (uint8_t) framed_byte(data, data_bytes, i);
}

template <bool STORE>
__global__ __launch_bounds__(kWave) void k_gif_encode(const EncodeArgs a, uint32_t* __restrict__ counts, const uint64_t* __restrict__ starts, uint8_t* __restrict__ out, uint64_t cap)
{
    __shared__ uint32_t s_slots[kHashSlots];
    __shared__ __attribute__((aligned(4))) uint8_t s_idx[kSegmentPixels];
    __shared__ uint16_t s_codes[STORE ? kSegmentPixels : 1];
    __shared__ uint32_t s_data[STORE ? kDataWords : 1];
    __shared__ uint32_t s_m;

    const int tid = (int) threadIdx.x, frame = (int) blockIdx.y;
    const uint32_t segment = blockIdx.x;
    const Geometry g = a.g;
    const uint32_t n = segment_length(g, segment);
    const bool first = segment == 0, last = segment + 1 == g.segments;
    const uint8_t* src = a.frames[frame];
    const uint64_t base = (uint64_t) segment * kSegmentPixels;
    for (uint32_t i = tid; i < n; i += kWave) s_idx[i] = a.lut[pixel_cell(src, g, base + i, true)];
    for (int i = tid; i < kHashSlots; i += kWave) s_slots[i] = Dictionary::kEmpty;
    if (STORE)
        for (int i = tid; i < kDataWords; i += kWave) s_data[i] = 0;
    __syncthreads();

    if (tid == 0) {
        Dictionary dict = { s_slots };
        if (STORE) { KeepCodes keep = { s_codes }; s_m = match_loop(s_idx, n, dict, keep); }
        else { CountCodes count; s_m = match_loop(s_idx, n, dict, count); }
    }
    __syncthreads();
    const uint32_t m = s_m;
    const uint32_t data_bytes = segment_data_bytes(m, first, last), bytes = framed_bytes(data_bytes);
    const size_t unit = (size_t) frame * (size_t) g.segments + segment;
    if (!STORE) {
        if (tid == 0) counts[unit] = bytes + (first ? (uint32_t) kLeadBytes : 0u) + (last ? (uint32_t) kTailBytes : 0u);
        return;
    }

    uint32_t pad;
    segment_bits(m, first, last, &pad);
    LdsWords words = { s_data };
    for (uint32_t j = (uint32_t) tid; j < m + 2u + pad; j += kWave) put_piece(words, s_codes, m, first, last, j);
    __syncthreads();

    uint64_t pos = starts[unit];
    if (first) {
        if (tid < kLeadBytes && pos + tid < cap) out[pos + tid] = a.lead[tid];
        pos += kLeadBytes;
    }
    const LdsData data = { s_data };
    store_framed(out, pos, cap, data, data_bytes, bytes);
    if (last && tid == 0 && pos + bytes < cap) out[pos + bytes] = 0x00;
}

struct HistogramArgs {
    const uint8_t* frames[kFramesPerLaunch];
    Geometry g;
};

__global__ __launch_bounds__(kBlock) void k_gif_histogram(const HistogramArgs a, uint32_t* __restrict__ hist)
{
    const Geometry g = a.g;
    const uint64_t at = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (at < g.pixels) atomicAdd(&hist[pixel_cell(a.frames[blockIdx.y], g, at, false)], 1u);
}

__global__ __launch_bounds__(kBlock) void k_gif_lut(const uint8_t* __restrict__ palette, int n_colors, uint8_t* __restrict__ lut)
{
    __shared__ uint8_t s_palette[3 * 256];
    for (int i = (int) threadIdx.x; i < 3 * n_colors; i += kBlock) s_palette[i] = palette[i];
    __syncthreads();
    const unsigned cell = blockIdx.x * kBlock + threadIdx.x;
    if (cell < (unsigned) kCells) lut[cell] = (uint8_t) nearest_entry(s_palette, n_colors, cell);
}

}  // namespace

extern "C" {

KBE_GIF_API int kbe_gif_abi_version(void)
{
    return KBE_GIF_ABI_VERSION;
}

KBE_GIF_API size_t kbe_gif_bound(int W, int H)
{
    return unit_bound(W, H);
}

KBE_GIF_API size_t kbe_gif_scratch_bytes(int W, int H, int n_frames)
{
    return unit_bound(W, H) && n_frames > 0 ? units_layout(geometry(W, H, 0, 0, 0).segments, n_frames, 0).bytes : 0;
}

KBE_GIF_API int kbe_gif_encode(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int flags, int dither, int delay_cs, const uint8_t* lut,
                               void* scratch, uint8_t* out, size_t cap, uint64_t* offsets, int* status, kbe_stream_t stream)
{
    const UnitsCall c = { "kbe_gif_encode", frames_u8, n_frames, W, H, scratch, out, cap, offsets, status, (hipStream_t) stream };
    const int rc = units_check(c, [&]() -> const char* {
        if (unit_bound(W, H) == 0) return "a frame's unit would not stay below 2^31 bytes";
        if (!(stride_bytes >= 3 * W && (flags & ~KBE_GIF_BGR) == 0)) return "bad stride or flags";
        if (dither < 0 || dither > kMaxDither) return "dither outside 0..64";
        if (delay_cs < 0 || delay_cs > 65535) return "delay_cs outside 0..65535";
        return lut ? nullptr : "null lut";
    });
    if (rc != KBE_OK) return rc;

    EncodeArgs a;
    a.g = geometry(W, H, stride_bytes, flags, dither);
    a.lut = lut;
    lead_bytes(W, H, delay_cs, a.lead);
    a.lead[kLeadBytes] = 0;
    return units_encode(c, a, (int) a.g.segments, 0, [&](bool store, int, int nf, uint32_t* counts, const uint64_t* starts, uint32_t*) {
        const dim3 grid(a.g.segments, (unsigned) nf);
        if (!store) hipLaunchKernelGGL(k_gif_encode<false>, grid, dim3(kWave), 0, c.s, a, counts, starts, out, (uint64_t) cap);
        else hipLaunchKernelGGL(k_gif_encode<true>, grid, dim3(kWave), 0, c.s, a, counts, starts, out, (uint64_t) cap);
    });
}

KBE_GIF_API int kbe_gif_histogram(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int flags, uint32_t* hist, kbe_stream_t stream)
{
    const char* what = nullptr;
    if (!(frames_u8 && n_frames >= 1 && W > 0 && H > 0 && W <= 65535 && H <= 65535)) what = "bad frames or size";
    else if (!(stride_bytes >= 3 * W && (flags & ~KBE_GIF_BGR) == 0)) what = "bad stride or flags";
    else if (!hist || ((uintptr_t) hist & 3) != 0) what = "bad hist";
    for (int i = 0; !what && i < n_frames; i++)
        if (!frames_u8[i]) what = "null frame";
    if (what) { snprintf(g_err, sizeof(g_err), "kbe_gif_histogram: %s", what); return KBE_E_INVALID; }
    HistogramArgs a;
    a.g = geometry(W, H, stride_bytes, flags, 0);
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = n_frames - f0 < kFramesPerLaunch ? n_frames - f0 : kFramesPerLaunch;
        for (int i = 0; i < kFramesPerLaunch; i++) a.frames[i] = i < nf ? frames_u8[f0 + i] : nullptr;
        hipLaunchKernelGGL(k_gif_histogram, dim3(blocks_for((size_t) a.g.pixels), (unsigned) nf), dim3(kBlock), 0, (hipStream_t) stream, a, hist);
    }
    return launched("kbe_gif_histogram");
}

KBE_GIF_API int kbe_gif_lut(const uint8_t* palette, int n_colors, uint8_t* lut, kbe_stream_t stream)
{
    if (!(palette && lut && n_colors >= 1 && n_colors <= 256)) { snprintf(g_err, sizeof(g_err), "kbe_gif_lut: %s", palette && lut ? "n_colors outside 1..256" : "null palette or lut"); return KBE_E_INVALID; }
    hipLaunchKernelGGL(k_gif_lut, dim3(kCells / kBlock), dim3(kBlock), 0, (hipStream_t) stream, palette, n_colors, lut);
    return launched("kbe_gif_lut");
}

}  // extern "C"
