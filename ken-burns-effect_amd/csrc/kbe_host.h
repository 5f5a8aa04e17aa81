// kbe_host.h -- host-side helpers shared by the translation units of libkbe_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "kbe.h"
#include "kbe_device.h"

namespace kbe {

extern thread_local char g_err[256];      // defined in kbe_hip.hip; read through kbe_last_error()

inline int fail(int code, const char* what, hipError_t e = hipSuccess)
{
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : "");
    return code;
}

inline int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? KBE_OK : fail(KBE_E_LAUNCH, what, e);
}

inline Camera make_camera(int W, int H, double focal, double baseline, const float* shift3)
{
    Camera c;
    c.focal_f = (float) focal;
    c.fb = focal * baseline;
    c.fb_f = (float) c.fb;
    c.half_w = 0.5 * (double) W;
    c.half_h = 0.5 * (double) H;
    c.cx_f = (float) (c.half_w - 0.5);
    c.cy_f = (float) (c.half_h - 0.5);
    c.fp32_centre = W >= 2 && H >= 2 && (double) c.cx_f == c.half_w - 0.5 && (double) c.cy_f == c.half_h - 0.5;
    c.W = W;
    c.H = H;
    c.has_shift = shift3 != nullptr;
    c.sx = shift3 ? shift3[0] : 0.0f;
    c.sy = shift3 ? shift3[1] : 0.0f;
    c.sz = shift3 ? shift3[2] : 0.0f;
    return c;
}

constexpr int kBlock = 256;

inline unsigned blocks_for(size_t n, int per_block = kBlock)
{
    return (unsigned) ((n + per_block - 1) / per_block);
}

// -- the frame filters' entries (kbe_area.hip .. kbe_sharpen.hip): each lists its own checks, in its own order; their mechanics are here --

// a refused call: "<entry>: <what>" for kbe_last_error()
inline int refuse(const char* entry, const char* what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, what);
    return KBE_E_INVALID;
}

// the bytes from a frame's first to one past its last: H rows `stride` bytes apart, row_bytes of each
inline uintptr_t frame_extent(int H, uintptr_t stride, uintptr_t row_bytes)
{
    return (uintptr_t) (H - 1) * stride + row_bytes;
}

struct Range {
    uintptr_t first, end;
};

inline bool intersect(const Range& a, const Range& b)
{
    return a.first < b.end && b.first < a.end;
}

// whether any of the na buffers a[i], a_bytes each, shares a byte with any of the nb buffers b[j], b_bytes each
template <class A, class B>
inline bool any_overlap(A* const* a, size_t na, uintptr_t a_bytes, B* const* b, size_t nb, uintptr_t b_bytes)
{
    for (size_t i = 0; i < na; i++)
        for (size_t j = 0; j < nb; j++)
            if (intersect(Range{(uintptr_t) a[i], (uintptr_t) a[i] + a_bytes}, Range{(uintptr_t) b[j], (uintptr_t) b[j] + b_bytes})) return true;
    return false;
}

// ... and whether any two of the n buffers a[i] do
template <class A>
inline bool any_two_overlap(A* const* a, size_t n, uintptr_t bytes)
{
    for (size_t i = 0; i + 1 < n; i++)
        if (any_overlap(a + i, 1, bytes, a + i + 1, n - i - 1, bytes)) return true;
    return false;
}

// A call's n frames are cut into launches of at most `most` each: how many the launch that begins at frame f0 carries ...
inline int launch_frames(int n, int f0, int most)
{
    return n - f0 < most ? n - f0 : most;
}

// ... and its pointer slots: table[first .. first + count), the rest nullptr
template <class T, int N>
inline void fill_slots(T* (&slots)[N], T* const* table, size_t first, int count)
{
    for (int i = 0; i < N; i++) slots[i] = i < count ? table[first + i] : nullptr;
}

}  // namespace kbe

#define KBE_REQUIRE(cond, what) do { if (!(cond)) return kbe::fail(KBE_E_INVALID, what); } while (0)
