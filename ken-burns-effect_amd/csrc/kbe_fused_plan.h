// What launch_frames_fused (kbe_fused.hip) decides before it enqueues anything: which consecutive frames of a group share candidate
// lists and by how much their boxes widen (share_plan), whether a tile launch can carry the next launch's placements, and which of
// the k_frame* kernels it is -- on plain values.  Plain C++ (no HIP): tests/fused_plan_check.cpp checks it on the host.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "kbe_cloud.h"

namespace kbe {

// the launch's geometry as plain values (kbe_fused.hip fills it from kbe_tiles.h's constants)
struct FusedGrid {
    int Np;                 // points of the packed cloud, padding included (cloud_layout_base)
    int tiles;              // tiles of a frame
    int waves_per_tile;     // waves of a tile's workgroup
    int list_cap;           // sub-blocks a tile's candidate list holds
};

// ---- shared candidate lists
constexpr int SHARE_MAX_FRAMES = 12;        // the largest sub-group: a launch takes no more frames (kbe_tiles.h: KBE_FRAME_JOBS)
#ifndef KBE_SHARE_MAX_PX
#define KBE_SHARE_MAX_PX 13.0
#endif
// frame k of a group reads the lists of frame lead[k] (itself: lists of its own), which serve frames lead[k] .. last[k] (size[k] of
// them); dev: the largest distance, per axis, of a camera's shift from the chord of its sub-group
struct SharePlan { bool any; float dev[3]; uint8_t lead[SHARE_MAX_FRAMES], last[SHARE_MAX_FRAMES], size[SHARE_MAX_FRAMES]; };

// Which consecutive frames of a group placed ahead share ONE set of candidate lists (kbe_fused.hip: FrameJobsT, ShareMode).
// The group's cameras (cam(0) .. cam(m - 1); the fields read: focal_f, fb, half_w, half_h, W, H, fp32_centre, has_shift, sx, sy, sz)
// must differ in their shifts only.  The frames are cut into sub-groups of s consecutive ones -- the
// largest s of 12, 8, 6, 4 for which the nearest point the caller knows of (`near_depth`: objectDepthrange's closest
// depth, common.py:88) moves by at most KBE_SHARE_MAX_PX pixels between a sub-group's first and last camera: a sub-block is
// listed for the box of its corners under those two cameras, and what the box gains in tiles must stay below what ONE list
// for s frames saves (measured).  A camera between the two need not lie on the straight line between
// them (a Ken Burns path is a parabola in shift space: shiftX = dU closestDepth(step) / F, common.py:88-100): how far the
// sub-groups' cameras stray from their chords goes to the kernel as `dev` and widens the boxes.  Decided from the group's
// cameras, the cloud and near_depth alone, so that the launch that places a group and the launch that renders it agree
// without being told.
template <class CamOf>
SharePlan share_plan(CamOf cam, int m, double near_depth, const FusedGrid& grid)
{
    SharePlan P = {};
    for (int k = 0; k < SHARE_MAX_FRAMES; k++) { P.lead[k] = P.last[k] = (uint8_t) k; P.size[k] = 1; }
    if (m < 2 || !(near_depth > 0.0)) return P;
    // a sub-group's list is longer than a frame's own, and a list beyond the capacity sends its tile down the slow path: only
    // clouds whose AVERAGE list (1.55 candidates per point of the tile's share, in sub-blocks) leaves a factor of four to
    // the capacity share (the bench cloud: 54 of 2048; 16.8 M points on 2048^2: 198, its densest tiles 480-500 -- with
    // lists of 512, until round 5, shared lists reached 515-555 there and eighteen tiles of a video scanned the whole cloud;
    // with 2048 such a cloud may share: measured the same with and without, 288.7 us per frame)
    if (1.55 * (double) grid.Np / kCloudSub / (double) grid.tiles > grid.list_cap / 4.0) return P;
    const auto& c0 = cam(0);
    double big = 1.0;
    for (int k = 0; k < m; k++) {
        const auto& c = cam(k);
        if (c.focal_f != c0.focal_f || c.fb != c0.fb || c.half_w != c0.half_w || c.half_h != c0.half_h || c.W != c0.W || c.H != c0.H ||
            c.fp32_centre != c0.fp32_centre || !c.has_shift || !c0.fp32_centre) return P;
        big = fmax(big, fmax(fabs((double) c.sx), fmax(fabs((double) c.sy), fabs((double) c.sz))));
    }
    if (big > 100.0) return P;
    const double F = (double) c0.focal_f, half = 0.5 * (double) (c0.W > c0.H ? c0.W : c0.H);
    auto spread_px = [&](int a, int b) {            // how far the nearest point moves between cameras a and b, in pixels
        const auto& ca = cam(a); const auto& cb = cam(b);
        const double zn = near_depth + fmin((double) ca.sz, (double) cb.sz);
        if (!(zn > 0.01 * F)) return 1.0e30;
        return (hypot((double) cb.sx - ca.sx, (double) cb.sy - ca.sy) * F + half * fabs((double) cb.sz - ca.sz)) / zn;
    };
    static const int sizes[] = { 12, 8, 6, 4 };         // (sub-groups of 2 or 3 measured slower than lists of their own: 17.4-17.7 against 16.8-17.0 us per frame)
    int s_sub = 0;
    for (int q = 0; q < 4 && !s_sub; q++) {
        const int sz = sizes[q] < m ? sizes[q] : m;
        if (sz < 4) break;                              // (a group of two or three frames: lists of their own)
        bool fits = true;
        for (int a0 = 0; a0 < m && fits; a0 += sz) { const int b0 = (a0 + sz < m ? a0 + sz : m) - 1; fits = b0 == a0 || spread_px(a0, b0) <= (double) KBE_SHARE_MAX_PX; }
        if (fits) s_sub = sz;
    }
    if (!s_sub) return P;
    // how far the cameras of a sub-group stray from its chord, per axis (+ the shifts' own fp32 rounding)
    double dev[3] = { 0.0, 0.0, 0.0 };
    for (int a0 = 0; a0 < m; a0 += s_sub) {
        const int b0 = (a0 + s_sub < m ? a0 + s_sub : m) - 1;
        const auto& ca = cam(a0); const auto& cb = cam(b0);
        const double d[3] = { (double) cb.sx - ca.sx, (double) cb.sy - ca.sy, (double) cb.sz - ca.sz };
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (int k = a0 + 1; k < b0; k++) {
            const auto& c = cam(k);
            const double e[3] = { (double) c.sx - ca.sx, (double) c.sy - ca.sy, (double) c.sz - ca.sz };
            double lam = dd > 0.0 ? (e[0] * d[0] + e[1] * d[1] + e[2] * d[2]) / dd : 0.0;
            lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
            for (int q = 0; q < 3; q++) dev[q] = fmax(dev[q], fabs(e[q] - lam * d[q]));
        }
    }
    for (int q = 0; q < 3; q++) dev[q] += 2.0e-6 * big;
    // (a path that strays from its chords by more than a pixel's worth at the nearest depth is no path to share lists on)
    const double zn0 = near_depth + fmin((double) c0.sz, (double) cam(m - 1).sz);
    if (!(zn0 > 0.01 * F) || (hypot(dev[0], dev[1]) * F + half * dev[2]) / zn0 > 2.0) return P;
    for (int a0 = 0; a0 < m; a0 += s_sub) {
        const int b0 = (a0 + s_sub < m ? a0 + s_sub : m) - 1;
        for (int k = a0; k <= b0; k++) { P.lead[k] = (uint8_t) a0; P.last[k] = (uint8_t) b0; P.size[k] = (uint8_t) (b0 - a0 + 1); }
        P.any = P.any || b0 > a0;
    }
    for (int q = 0; q < 3; q++) P.dev[q] = (float) (dev[q] * 1.0001);
    return P;
}

// ---- placements ahead
// Can the tile launch of n frames make the placements of n_next frames without outliving its own work?  Its waves share them:
// up to a few units of 64 points per wave (beyond KBE_AHEAD_UNITS + 1 per wave the launch is k_frame_group_ahead_dense).
#ifndef KBE_AHEAD_UNITS
#define KBE_AHEAD_UNITS 3       // units a wave places up front (a wave's share of an equal group is 2.17 units: with three up front nothing is left for the end; 17.9 -> 17.6 us per frame)
#endif
#ifndef KBE_AHEAD_MAX_UNITS
#define KBE_AHEAD_MAX_UNITS 9
#endif
inline size_t ahead_units_per_wave(const FusedGrid& grid, int n, int n_next)        // rounded up
{
    const size_t units = (size_t) grid.Np / kCloudBlock * (size_t) n_next;
    const size_t waves = (size_t) grid.tiles * grid.waves_per_tile * (size_t) n;
    return (units + waves - 1) / waves;
}
inline bool fused_can_place_ahead(const FusedGrid& grid, int n, int n_next)
{
    if (n < 1 || n_next < 1) return false;
    return ahead_units_per_wave(grid, n, n_next) <= (size_t) KBE_AHEAD_MAX_UNITS;
}

// ---- the kernel of a tile launch
#ifndef KBE_LEAN_MAX_DENSITY
#define KBE_LEAN_MAX_DENSITY 1.125
#endif
enum class FusedShape { SINGLE, SINGLE_AHEAD, GROUP, GROUP_AHEAD };    // one frame (FrameJob1) or a group (FrameJobs); AHEAD: it also makes placements
enum class FusedBuild { LEAN, ROOMY, DENSE };                           // kbe_fused.hip: "Two builds of every tile launch", and k_frame_group_ahead_dense
struct FusedKernel { FusedShape shape; FusedBuild build; };
// the tile launch of n frames of W x H that makes the placements of n_next: the lean build (608 records per tile, six workgroups per
// CU) for clouds of about a point per pixel, the roomy one beyond (`forced`: 1 = lean, 2 = roomy -- a switch for tests and
// measurements); a group whose waves place more than KBE_AHEAD_UNITS + 1 units each takes the dense launch, which has one build
inline FusedKernel fused_kernel(const FusedGrid& grid, int W, int H, int n, int n_next, int forced)
{
    const bool lean = forced ? forced == 1 : (double) grid.Np <= KBE_LEAN_MAX_DENSITY * (double) W * (double) H;
    const FusedBuild build = lean ? FusedBuild::LEAN : FusedBuild::ROOMY;
    if (n == 1 && n_next <= 1) return FusedKernel{ n_next ? FusedShape::SINGLE_AHEAD : FusedShape::SINGLE, build };
    if (!n_next) return FusedKernel{ FusedShape::GROUP, build };
    const bool dense = ahead_units_per_wave(grid, n, n_next) > (size_t) KBE_AHEAD_UNITS + 1;        // (also: one frame that places several)
    return FusedKernel{ FusedShape::GROUP_AHEAD, dense ? FusedBuild::DENSE : build };
}

}  // namespace kbe
