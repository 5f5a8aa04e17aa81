// kbe_png.hip -- kbe_png_encode: frames that lie in HBM as PNG files, back to back, for the frame writer (include/kbe.h).  The file and
// all of its arithmetic are defined in kbe_png_block.h; this file spreads that work over the chip.
//
// A frame's segments (kSegmentBytes filtered bytes each) are independent, but where a segment's bytes go depends on the lengths of all
// segments in front of it.  So the work is done twice, with nothing but 24 bytes per segment in HBM between the two passes:
//   1. k_png_encode<false>: a workgroup takes one segment: the filtered bytes into LDS; every lane looks at a piece of kPieceBytes of them,
//      and two scans across the workgroup tell it where the run that reaches into its piece starts and where the run that leaves it ends
//      -- the tokens are then kbe_png_block.h's closed form; their histogram in LDS; the used symbols ranked one per lane; ONE lane
//      builds the two codes and the block header (the header's functions, as they are); the tokens' bit lengths summed: the segment's
//      LENGTH, coded or stored, is all that is written;
//   2. the exclusive scan of the lengths over all segments of all frames of the launch (kbe_units_scan.h): every segment's place, every
//      frame's offsets[i], the total and `status`;
//   3. k_png_encode<true>: the same again, then every lane packs its piece's bits at their place (a prefix sum of the bit lengths) into
//      LDS words, the workgroup copies the bytes to their place in HBM (nothing at or beyond `cap`), and leaves three words per segment:
//      its share of the two Adler-32 sums and its raw CRC-32 advanced to the end of the IDAT;
//   4. k_png_tail: a workgroup per frame adds those up and writes the frame's first 43 bytes (the IDAT's length) and last 22.
// No kernel waits for another workgroup.  n frames are cut into launches of kFramesPerLaunch.
#include "kbe_host.h"
#include "kbe_png_block.h"
#include "kbe_units_scan.h"

using namespace kbe;
using namespace kbe_png;

namespace {

constexpr int kEncodeThreads = 256;
constexpr int kPieceBytes = kSegmentBytes / kEncodeThreads;                     // a lane's piece of a segment
constexpr int kOutWords = (kSegmentBytes + 5 + 3) / 4 + 1;                      // a segment's bytes are at most its stored form's
constexpr int kMarkWords = 3;                                                   // per segment: Adler a, Adler b, CRC
static_assert(kSegmentBytes % kEncodeThreads == 0, "whole pieces");

struct EncodeArgs {
    const uint8_t* frames[kFramesPerLaunch];
    Geometry g;
    Powers pw;
    uint8_t lead[kLeadBytes + 1];
};
static_assert(sizeof(EncodeArgs) <= 3840, "kernel arguments: 4 KB at most");

// kbe_png_block.h's WordBits on LDS words: the OR is atomic
struct LdsWords {
    uint32_t* w;
    __device__ __forceinline__ void merge(uint32_t index, uint32_t value) { atomicOr(&w[index], value); }
};
typedef WordBits<LdsWords> AtomicBits;

struct AtomicHistogram {
    uint32_t* hist;
    __device__ __forceinline__ void token(int kind, unsigned byte)
    {
        if (kind == 1) atomicAdd(&hist[byte], 1u);
        else if (kind) { int sym, eb; unsigned extra; length_symbol(kind, &sym, &eb, &extra); atomicAdd(&hist[sym], 1u); }
    }
};

// n bytes from LDS to files[pos ...), by the whole workgroup, StoreSink's rule (kbe_mjpeg.hip): singly up to the first 4-byte boundary, then
// four at a time, the rest singly; never at or beyond cap
__device__ __forceinline__ void store_bytes(uint8_t* files, uint64_t pos, uint64_t cap, const uint8_t* from, uint32_t n)
{
    const uint32_t tid = threadIdx.x;
    uint32_t head = (4u - (uint32_t) (((uintptr_t) files + pos) & 3u)) & 3u;
    if (head > n) head = n;
    if (tid < head && pos + tid < cap) files[pos + tid] = from[tid];
    const uint32_t words = (n - head) / 4u;
    for (uint32_t j = tid; j < words; j += kEncodeThreads) {
        const uint32_t at = head + 4u * j;
        const uint64_t p = pos + at;
        if (p + 4 <= cap)
            *reinterpret_cast<uint32_t*>(files + p) = (uint32_t) from[at] | ((uint32_t) from[at + 1] << 8) | ((uint32_t) from[at + 2] << 16) | ((uint32_t) from[at + 3] << 24);
        else
            for (uint32_t k = 0; k < 4; k++)
                if (p + k < cap) files[p + k] = from[at + k];
    }
    for (uint32_t i = head + 4u * words + tid; i < n; i += kEncodeThreads)
        if (pos + i < cap) files[pos + i] = from[i];
}

template <bool STORE>
__global__ __launch_bounds__(kEncodeThreads) void k_png_encode(const EncodeArgs a, uint32_t* __restrict__ counts, const uint64_t* __restrict__ starts,
                                                               const uint64_t* __restrict__ offsets, int f0, uint32_t* __restrict__ marks, uint8_t* __restrict__ files, uint64_t cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_b[kSegmentBytes];
    __shared__ __attribute__((aligned(16))) uint32_t s_out[STORE ? kOutWords : 1];
    __shared__ uint32_t s_crc[STORE ? 256 : 1], s_x8[STORE ? 32 : 1];
    __shared__ Work s_w;
    __shared__ uint32_t s_left[kEncodeThreads], s_right[kEncodeThreads];
    __shared__ uint32_t s_used, s_header_bits, s_adler_a, s_adler_b, s_crc_sum;

    const int tid = (int) threadIdx.x, frame = (int) blockIdx.y;
    const uint32_t segment = blockIdx.x;
    const Geometry g = a.g;
    const uint32_t n = segment_length(g, segment), base = segment * (uint32_t) kSegmentBytes;
    const uint8_t* src = a.frames[frame];
    for (uint32_t i = tid; i < n; i += kEncodeThreads) s_b[i] = (uint8_t) filtered_byte(src, g, base + i);
    for (int i = tid; i < kLitSyms; i += kEncodeThreads) s_w.hist[i] = 0;
    if (STORE) {
        for (int i = tid; i < kOutWords; i += kEncodeThreads) s_out[i] = 0;
        s_crc[tid] = crc_table_entry((unsigned) tid);
        if (tid < 32) s_x8[tid] = a.pw.x8[tid];
    }
    if (tid == 0) { s_used = 0; s_adler_a = 0; s_adler_b = 0; s_crc_sum = 0; }
    __syncthreads();

    // where runs start in this lane's piece: the last such place (+ 1; 0: none) for the lanes behind, the first (n: none) for the lanes in front
    const int begin = (int) (tid * kPieceBytes < (int) n ? tid * kPieceBytes : (int) n), end = (int) (begin + kPieceBytes < (int) n ? begin + kPieceBytes : (int) n);
    {
        uint32_t last = 0, first = n;
        for (int p = begin; p < end; p++)
            if (p == 0 || s_b[p] != s_b[p - 1]) { if (first == n) first = (uint32_t) p; last = (uint32_t) p + 1u; }
        s_left[tid] = last;
        s_right[tid] = first;
    }
    __syncthreads();
    for (int d = 1; d < kEncodeThreads; d <<= 1) {
        const uint32_t l = tid >= d ? s_left[tid - d] : 0u, r = tid + d < kEncodeThreads ? s_right[tid + d] : n;
        __syncthreads();
        if (l > s_left[tid]) s_left[tid] = l;
        if (r < s_right[tid]) s_right[tid] = r;
        __syncthreads();
    }
    const bool starts_here = begin < end && (begin == 0 || s_b[begin] != s_b[begin - 1]);
    const int start = starts_here || tid == 0 ? begin : (int) s_left[tid - 1] - 1;
    const int next = tid + 1 < kEncodeThreads ? (int) s_right[tid + 1] : (int) n;

    // the tokens' histogram, the used symbols in order
    {
        AtomicHistogram h = { s_w.hist };
        walk(s_b, begin, end, start, next, h);
        if (tid == 0) atomicAdd(&s_w.hist[kEob], 1u);
    }
    __syncthreads();
    for (int i = tid; i < kLitSyms; i += kEncodeThreads)
        if (s_w.hist[i]) { s_w.order[rank_of(s_w.hist, kLitSyms, i)] = (uint16_t) i; atomicAdd(&s_used, 1u); }
    __syncthreads();

    // one lane: the codes and the block header
    if (tid == 0) {
        s_w.used = (int) s_used;
        s_w.limited = lengths_from_order(s_w.hist, s_w.order, s_w.used, kLitSyms, kLitLimit, s_w.lit_len, s_w.weight, s_w.up, s_w.count);
        canonical_codes(s_w.lit_len, kLitSyms, kLitLimit, s_w.lit_code, s_w.count, s_w.next);
        if (STORE) {
            AtomicBits header = { { s_out }, 0, 0, 0 };
            header.start(0u);
            block_header(&s_w, header);
            header.finish();
            s_header_bits = header.position();
        } else {
            CountBits header = { 0u };
            block_header(&s_w, header);
            s_header_bits = header.n;
        }
    }
    __syncthreads();

    // the tokens' bits: this lane's, then a prefix sum over the lanes
    LengthOut mine = { &s_w, 0u };
    walk(s_b, begin, end, start, next, mine);
    s_left[tid] = mine.n;
    __syncthreads();
    for (int d = 1; d < kEncodeThreads; d <<= 1) {
        const uint32_t below = tid >= d ? s_left[tid - d] : 0u;
        __syncthreads();
        s_left[tid] += below;
        __syncthreads();
    }
    const uint32_t before = s_left[tid] - mine.n, tokens_bits = s_left[kEncodeThreads - 1], header_bits = s_header_bits;
    const uint32_t coded = coded_bytes(&s_w, header_bits, tokens_bits);
    const bool stored = coded >= n + 5u;
    const uint32_t bytes = stored ? n + 5u : coded;
    const uint32_t lead = segment == 0 ? (uint32_t) kLeadBytes : 0u, tail = segment + 1 == g.segments ? (uint32_t) kTailBytes : 0u;
    const size_t unit = (size_t) frame * (size_t) g.segments + segment;
    if (!STORE) {
        if (tid == 0) counts[unit] = bytes + lead + tail;
        return;
    }

    uint8_t* out = reinterpret_cast<uint8_t*>(s_out);
    if (stored) {
        // (the header's bits lie in s_out: the stored form is written over them)
        for (uint32_t i = tid; i < n; i += kEncodeThreads) out[5 + i] = s_b[i];
        if (tid == 0) { out[0] = 0; out[1] = (uint8_t) n; out[2] = (uint8_t) (n >> 8); out[3] = (uint8_t) ~n; out[4] = (uint8_t) (~n >> 8); }
    } else {
        AtomicBits packed = { { s_out }, 0, 0, 0 };
        packed.start(header_bits + before);
        PackOut<AtomicBits> pack = { &s_w, packed };
        walk(s_b, begin, end, start, next, pack);
        packed.finish();
        if (tid == 0) {
            AtomicBits last = { { s_out }, 0, 0, 0 };
            last.start(header_bits + tokens_bits);
            end_coded(&s_w, last, header_bits + tokens_bits);
            last.finish();
        }
    }
    __syncthreads();

    const uint64_t pos = starts[unit] + lead;
    store_bytes(files, pos, cap, out, bytes);

    // the check sums' pieces: this lane's part of the segment's bytes, advanced to the end of the IDAT's data; its piece of the filtered bytes
    {
        const uint64_t behind = (offsets[f0 + frame + 1] - 16u) - (pos + bytes);
        const uint32_t per_lane = (bytes + kEncodeThreads - 1) / kEncodeThreads;
        const uint32_t p0 = (uint32_t) tid * per_lane < bytes ? (uint32_t) tid * per_lane : bytes, p1 = p0 + per_lane < bytes ? p0 + per_lane : bytes;
        if (p1 > p0) atomicXor(&s_crc_sum, crc_advance(s_x8, crc_raw(s_crc, out + p0, p1 - p0), behind + (bytes - p1)));
        if (end > begin) {
            uint32_t pa, pb;
            adler_piece(s_b + begin, (uint32_t) (end - begin), g.raw - ((uint64_t) base + (uint32_t) end), &pa, &pb);
            atomicAdd(&s_adler_a, pa);
            atomicAdd(&s_adler_b, pb);
        }
    }
    __syncthreads();
    if (tid == 0) {
        marks[unit * kMarkWords + 0] = s_adler_a;           // (256 terms below 65521 each)
        marks[unit * kMarkWords + 1] = s_adler_b;
        marks[unit * kMarkWords + 2] = s_crc_sum;
    }
}

// a workgroup per frame: the segments' marks added up, the frame's first kLeadBytes and last kTailBytes written (nothing at or beyond cap)
__global__ __launch_bounds__(kEncodeThreads) void k_png_tail(const EncodeArgs a, const uint32_t* __restrict__ marks, const uint64_t* __restrict__ offsets, int f0,
                                                             uint8_t* __restrict__ files, uint64_t cap)
{
    __shared__ uint32_t s_crc[256], s_x8[32];
    __shared__ uint32_t s_a, s_b, s_c;
    __shared__ uint8_t s_lead[kLeadBytes + 1], s_tail[kTailBytes + 2];
    const int tid = (int) threadIdx.x, frame = (int) blockIdx.x;
    const Geometry g = a.g;
    s_crc[tid] = crc_table_entry((unsigned) tid);
    if (tid < 32) s_x8[tid] = a.pw.x8[tid];
    if (tid == 0) { s_a = 0; s_b = 0; s_c = 0; }
    __syncthreads();
    uint64_t sa = 0, sb = 0;
    uint32_t sc = 0;
    for (uint32_t s = (uint32_t) tid; s < g.segments; s += kEncodeThreads) {
        const uint32_t* m = marks + ((size_t) frame * g.segments + s) * kMarkWords;
        sa += m[0];
        sb += m[1];
        sc ^= m[2];
    }
    atomicAdd(&s_a, (uint32_t) (sa % kAdlerMod));
    atomicAdd(&s_b, (uint32_t) (sb % kAdlerMod));
    atomicXor(&s_c, sc);
    __syncthreads();
    const uint64_t at = offsets[f0 + frame], size = offsets[f0 + frame + 1] - at;
    if (tid == 0) {
        for (int i = 0; i < kLeadBytes; i++) s_lead[i] = a.lead[i];
        lead_length(s_lead, size);
        tail_bytes(s_x8, s_crc, g.raw, s_a, s_b, s_c, size, s_tail);
    }
    __syncthreads();
    if (tid < kLeadBytes && at + tid < cap) files[at + tid] = s_lead[tid];
    if (tid < kTailBytes && at + size - kTailBytes + tid < cap) files[at + size - kTailBytes + tid] = s_tail[tid];
}

}  // namespace

extern "C" {

size_t kbe_png_bound(int W, int H)
{
    return file_bound(W, H);
}

size_t kbe_png_scratch_bytes(int W, int H, int n_frames)
{
    return file_bound(W, H) && n_frames > 0 ? units_layout(geometry(W, H, 0, 0).segments, n_frames, kMarkWords).bytes : 0;
}

int kbe_png_encode(const uint8_t* const* frames_u8, int n_frames, int W, int H, int stride_bytes, int flags, void* scratch, uint8_t* files, size_t cap, uint64_t* offsets,
                   int* status, kbe_stream_t stream)
{
    const UnitsCall c = { "kbe_png_encode", frames_u8, n_frames, W, H, scratch, files, cap, offsets, status, (hipStream_t) stream };
    const int rc = units_check(c, [&]() -> const char* {
        if (file_bound(W, H) == 0) return "a frame's file would not stay below 2^31 bytes";
        return stride_bytes >= 3 * W && (flags & ~KBE_PNG_BGR) == 0 ? nullptr : "bad stride or flags";
    });
    if (rc != KBE_OK) return rc;

    EncodeArgs a;
    a.g = geometry(W, H, stride_bytes, flags);
    {
        host::Tables t;
        host::tables_build(W, H, &t);
        a.pw = t.pw;
        for (int i = 0; i <= kLeadBytes; i++) a.lead[i] = t.lead[i];
    }
    return units_encode(c, a, (int) a.g.segments, kMarkWords, [&](bool store, int f0, int nf, uint32_t* counts, const uint64_t* starts, uint32_t* marks) {
        const dim3 grid(a.g.segments, (unsigned) nf);
        if (!store) hipLaunchKernelGGL(k_png_encode<false>, grid, dim3(kEncodeThreads), 0, c.s, a, counts, starts, (const uint64_t*) offsets, f0, marks, files, (uint64_t) cap);
        else hipLaunchKernelGGL(k_png_encode<true>, grid, dim3(kEncodeThreads), 0, c.s, a, counts, starts, (const uint64_t*) offsets, f0, marks, files, (uint64_t) cap);
        if (store) hipLaunchKernelGGL(k_png_tail, dim3((unsigned) nf), dim3(kEncodeThreads), 0, c.s, a, (const uint32_t*) marks, (const uint64_t*) offsets, f0, files, (uint64_t) cap);
    });
}

}  // extern "C"
