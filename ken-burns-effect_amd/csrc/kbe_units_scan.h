// kbe_units_scan.h -- where the bytes of independently encoded UNITS go: the exclusive scan that the device-side encoders share
// (kbe_mjpeg.hip: a unit is a restart interval; kbe_png.hip: a segment).  counts[] holds the bytes of every unit of every frame of a launch,
// units_per_frame to a frame (a frame's first unit carries the bytes in front of it); three launches -- sums of kScanThreads, a scan of the
// sums, apply -- give every unit's place, every frame's offsets[i], the total and `status`.  No kernel waits for another workgroup.
// Kernels have internal linkage: every .hip file that includes this gets its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

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

}  // namespace
