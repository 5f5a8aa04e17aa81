// kbe_units_scan.h -- what the device-side encoders share (kbe_mjpeg.hip: a UNIT is a restart interval; kbe_png.hip: a segment): units are
// encoded independently, but where a unit's bytes go depends on the lengths of all units in front of it.  So an encoder runs twice -- a pass
// that counts, a pass that stores -- around the exclusive scan of this file: counts[] holds the bytes of every unit of every frame of a launch,
// units_per_frame to a frame (a frame's first unit carries the bytes in front of it); three launches -- sums of kScanThreads, a scan of the
// sums, apply -- give every unit's place, every frame's offsets[i], the total and `status`.  No kernel waits for another workgroup.
// Below the kernels, the host side of that, once: the scratch's layout, the checks of the contract's common arguments (include/kbe.h) and
// the loop that cuts n frames into launches; an encoder brings its kernel arguments and its two passes' launches.
// Kernels have internal linkage: every .hip file that includes this gets its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "kbe_host.h"

namespace {

constexpr int kFramesPerLaunch = 12;
constexpr int kScanThreads = 256;                                               // units per workgroup of the scan
constexpr int kSumsThreads = 64;                                                // sums the scan of the sums takes at once

// exclusive scan of one value per thread over a workgroup of THREADS; *total: the sum
template <int THREADS>
__device__ __forceinline__ uint64_t group_exclusive_scan(uint64_t v, uint64_t* lds, uint64_t* total)
{
    const int t = (int) threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const uint64_t below = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += below;
        __syncthreads();
    }
    const uint64_t inclusive = lds[t];
    *total = lds[THREADS - 1];
    __syncthreads();
    return inclusive - v;
}

__global__ __launch_bounds__(kScanThreads) void k_units_sums(const uint32_t* __restrict__ counts, size_t n, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[kScanThreads];
    const size_t at = (size_t) blockIdx.x * kScanThreads + threadIdx.x;
    uint64_t total;
    group_exclusive_scan<kScanThreads>(at < n ? counts[at] : 0u, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the sums become where their kScanThreads units start; offsets[f0] carries on from the launch before; the total and `status`
__global__ __launch_bounds__(kSumsThreads) void k_units_scan_sums(uint64_t* __restrict__ sums, size_t n_sums, uint64_t* __restrict__ offsets, int f0, int nf, uint64_t cap,
                                                                  int* __restrict__ status)
{
    __shared__ uint64_t lds[kSumsThreads];
    uint64_t carry = f0 == 0 ? 0 : offsets[f0];
    for (size_t at = 0; at < n_sums; at += kSumsThreads) {
        const size_t i = at + threadIdx.x;
        const uint64_t mine = i < n_sums ? sums[i] : 0;
        uint64_t total;
        const uint64_t before = group_exclusive_scan<kSumsThreads>(mine, lds, &total);
        if (i < n_sums) sums[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        offsets[f0 + nf] = carry;
        *status = carry > cap ? 1 : 0;              // (the totals grow from launch to launch: the last launch's word is the call's)
    }
}

__global__ __launch_bounds__(kScanThreads) void k_units_starts(const uint32_t* __restrict__ counts, size_t n, const uint64_t* __restrict__ sums, int units_per_frame,
                                                               uint64_t* __restrict__ starts, uint64_t* __restrict__ offsets, int f0)
{
    __shared__ uint64_t lds[kScanThreads];
    const size_t at = (size_t) blockIdx.x * kScanThreads + threadIdx.x;
    uint64_t total;
    const uint64_t start = sums[blockIdx.x] + group_exclusive_scan<kScanThreads>(at < n ? counts[at] : 0u, lds, &total);
    if (at < n) {
        starts[at] = start;
        if (at % (size_t) units_per_frame == 0) offsets[f0 + at / (size_t) units_per_frame] = start;       // a frame's first unit: where its bytes start
    }
}

// the scratch of a call: per unit of the largest launch a count (4 bytes), a start (8) and `extra_words` words of the encoder's own, and a
// sum per kScanThreads units; it does not grow past one launch's frames
struct UnitsLayout { size_t starts, sums, extra, bytes; };          // byte offsets; the counts lie at 0

inline UnitsLayout units_layout(size_t units_per_frame, int n_frames, int extra_words)
{
    const size_t n = (size_t) (n_frames < kFramesPerLaunch ? n_frames : kFramesPerLaunch) * units_per_frame;
    const size_t starts = (n * 4 + 7) & ~(size_t) 7, sums = starts + n * 8, extra = sums + ((n + kScanThreads - 1) / kScanThreads) * 8;
    return { starts, sums, extra, extra + n * (size_t) extra_words * 4 };
}

// the arguments every encoder takes (include/kbe.h), and the entry's name for its messages
struct UnitsCall { const char* entry; const uint8_t* const* frames_u8; int n_frames, W, H; void* scratch; uint8_t* out; size_t cap; uint64_t* offsets; int* status; hipStream_t s; };

// ... checked before anything is enqueued; own(): the entry's own checks (nullptr, or what is wrong), made once W and H are in range
template <class Own>
int units_check(const UnitsCall& c, Own own)
{
    const char* what = c.frames_u8 && c.n_frames >= 1 && c.W > 0 && c.H > 0 && c.W <= 65535 && c.H <= 65535 ? own() : "bad frames or size";
    if (!what && !(c.scratch && ((uintptr_t) c.scratch & 7) == 0 && c.offsets && ((uintptr_t) c.offsets & 7) == 0 && c.status && (c.out || c.cap == 0))) what = "bad buffers";
    for (int i = 0; !what && i < c.n_frames; i++)
        if (!c.frames_u8[i]) what = "null frame";
    if (what) snprintf(kbe::g_err, sizeof(kbe::g_err), "%s: %s", c.entry, what);
    return what ? KBE_E_INVALID : KBE_OK;
}

// n frames, kFramesPerLaunch to a launch: count, scan, store.  a: the encoder's kernel arguments, whose frames[kFramesPerLaunch] are filled in
// per launch; pass(store, f0, nf, counts, starts, extra) enqueues the encoder's counting (store false) or storing launches of frames f0 ... f0 + nf
template <class Args, class Pass>
int units_encode(const UnitsCall& c, Args& a, int units_per_frame, int extra_words, Pass pass)
{
    const UnitsLayout lay = units_layout((size_t) units_per_frame, c.n_frames, extra_words);
    uint32_t* counts = (uint32_t*) c.scratch;
    uint64_t* starts = (uint64_t*) ((char*) c.scratch + lay.starts);
    uint64_t* sums = (uint64_t*) ((char*) c.scratch + lay.sums);
    uint32_t* extra = (uint32_t*) ((char*) c.scratch + lay.extra);
    for (int f0 = 0; f0 < c.n_frames; f0 += kFramesPerLaunch) {
        const int nf = c.n_frames - f0 < kFramesPerLaunch ? c.n_frames - f0 : kFramesPerLaunch;
        for (int i = 0; i < kFramesPerLaunch; i++) a.frames[i] = i < nf ? c.frames_u8[f0 + i] : nullptr;
        const size_t n = (size_t) nf * (size_t) units_per_frame, n_sums = (n + kScanThreads - 1) / kScanThreads;
        pass(false, f0, nf, counts, (const uint64_t*) starts, extra);
        hipLaunchKernelGGL(k_units_sums, dim3((unsigned) n_sums), dim3(kScanThreads), 0, c.s, (const uint32_t*) counts, n, sums);
        hipLaunchKernelGGL(k_units_scan_sums, dim3(1), dim3(kSumsThreads), 0, c.s, sums, n_sums, c.offsets, f0, nf, (uint64_t) c.cap, c.status);
        hipLaunchKernelGGL(k_units_starts, dim3((unsigned) n_sums), dim3(kScanThreads), 0, c.s, (const uint32_t*) counts, n, (const uint64_t*) sums, units_per_frame, starts, c.offsets, f0);
        pass(true, f0, nf, counts, (const uint64_t*) starts, extra);
        const int rc = kbe::launched(c.entry);
        if (rc != KBE_OK) return rc;
    }
    return KBE_OK;
}

}  // namespace
