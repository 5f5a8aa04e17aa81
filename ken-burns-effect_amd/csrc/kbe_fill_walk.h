// kbe_fill_walk.h -- the exact arithmetic of the table-driven hole fill (kbe_holes.hip: k_hole_dist, k_fill_tables) and what
// launch_fill decides before it enqueues, each defined ONCE and compiled twice: by hipcc into the kernels, and by g++ into
// tests/fill_walk_check.cpp, which checks these very functions against brute force on the host (no hip_runtime.h, no
// kbe_tiles.h there: tile size and the box table's type come in as template parameters).  DESIGN.md section 4.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KBE_HD __host__ __device__ __forceinline__
#else
#define KBE_HD inline
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "kbe.h"

#pragma clang fp contract(off)

namespace kbe {

KBE_HD uint32_t f32_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
KBE_HD float bits_f32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
KBE_HD int imin(int a, int b) { return a < b ? a : b; }
KBE_HD int imax(int a, int b) { return a > b ? a : b; }
// 1 / v for a guess that a test follows (axis_catch_up).  The host's is deliberately sloppier than v_rcp_f32 -- fifty steps from a binade
// boundary the guess then overshoots by a step or more: the checker shows that the test is what counts
KBE_HD float rcp_guess(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(v);
#else
    return (1.0f / v) * 1.02f;
#endif
}

// ---------------------------------------------------------------------------------------
// m fp32 additions at once
// ---------------------------------------------------------------------------------------

// m repeated fp32 additions a := a - u (or + u), exactly, in a few steps.  While a stays in one binade [2^e, 2^(e+1))
// every value of the chain is a multiple of q = 2^(e-23), and each rounded sum moves a by the SAME amount R = u rounded to
// a multiple of q: the exact sum lies between two neighbours of a's grid, and which one is nearer does not depend on a --
// unless u sits exactly half-way between two multiples of q (a tie: round-to-even looks at a).  j such sums are a -/+ j R,
// computed on the integer mantissa.  j is cut so that the chain, and one step beyond it on either side, stays inside the
// binade (no sum is rounded on a finer or a coarser grid); across a binade boundary, for ties, below 1 and for the last
// two steps the sums are added one at a time.  (tests/fill_walk_check.cpp: against step-by-step sums.)
// `limit`: positions below -1 or above limit + 1 are outside the image for good (the ray is monotone), where the value
// no longer matters: the direction is skipped (common.py:880-885).
KBE_HD float advance_exact(float a, float u, int m, bool subtract, float limit)
{
    if (u == 0.0f) return a;
    while (m > 0) {
        const uint32_t bits = f32_bits(a);
        const int e = (int) (bits >> 23) - 127;
        if (m >= 3 && a >= 1.0f && e <= 23) {
            const float sc = ldexpf(u, 23 - e);                 // u / q, exact
            const float r = rintf(sc);
            if (fabsf(sc - r) != 0.5f) {
                const int step = (int) r, mag = abs(step);
                const int A = (int) ((bits & 0x7FFFFFu) | 0x800000u);       // a / q in [2^23, 2^24)
                const bool down = subtract ? step > 0 : step < 0;
                const int room_down = A - (1 << 23) - mag, room_up = (1 << 24) - 1 - mag - A;
                const int room = down ? room_down : room_up, other = down ? room_up : room_down;
                int j = (room > 0 && other >= 0 && mag > 0) ? (int) ((float) room / (float) mag) - 1 : 0;     // <= room / mag for sure
                j = imin(j, m);
                if (j >= 1) {
                    const int end = A + j * (down ? -mag : mag);
                    a = bits_f32((bits & 0xFF800000u) | ((uint32_t) end & 0x7FFFFFu));
                    m -= j;
                    continue;
                }
            }
        }
        a = subtract ? a - u : a + u;
        m--;
        if (a < -1.0f || a > limit) break;
    }
    return a;
}

// One coordinate of a ray end while it walks.  Fast mode (e >= 0): the coordinate is A 2^(e-23) with A in [2^23, 2^24),
// and one fp32 addition of -/+ u moves A by `step` (advance_exact's argument, kept as state): m additions are one
// multiply-add and one range test, the pixel a shift.  Invariant of the fast mode: A, and one step to either side of it,
// inside the binade.  Slow mode (e < 0; A holds the float's bits): below 32, next to a binade boundary, or a tie --
// single additions until the fast mode can be entered again.
struct Axis { int A, step, e; };

KBE_HD bool axis_interior(int A, int mag) { return (unsigned) (A - (1 << 23) - mag) < (unsigned) ((1 << 23) - 2 * mag); }

KBE_HD Axis axis_enter(float f, float u, bool subtract)
{
    const uint32_t bits = f32_bits(f);
    const int e = (int) (bits >> 23) - 127;
    if (f >= 32.0f && e <= 22) {                                // |step| <= 2^18: m * step cannot overflow, 2 |step| < 2^23
        const float sc = ldexpf(u, 23 - e);                     // u / q, exact
        const float r = rintf(sc);
        const int step = subtract ? -(int) r : (int) r;
        const int A = (int) ((bits & 0x7FFFFFu) | 0x800000u);
        if (fabsf(sc - r) != 0.5f && axis_interior(A, abs(step))) return Axis{ A, step, e };
    }
    return Axis{ (int) bits, 0, -1 };
}

KBE_HD float axis_value(const Axis& ax)
{
    return ax.e >= 0 ? bits_f32(((uint32_t) (ax.e + 127) << 23) | ((uint32_t) ax.A & 0x7FFFFFu)) : bits_f32((uint32_t) ax.A);
}

KBE_HD int axis_pixel(const Axis& ax)                           // (int) roundf(value): positive values round half up
{
    if (ax.e >= 0) { const int sh = 23 - ax.e; return (ax.A + (1 << (sh - 1))) >> sh; }
    return (int) roundf(bits_f32((uint32_t) ax.A));
}

// r pending additions, all at once if they end inside the binade (and the invariant holds at the end: everything in between
// lies between two interior values)
KBE_HD void axis_jump(Axis& ax, int& r)
{
    if (ax.e >= 0) {
        const int end = ax.A + r * ax.step;
        if (axis_interior(end, abs(ax.step))) { ax.A = end; r = 0; }
    }
}

// ... otherwise, typically in front of a binade boundary: as many as fit in front of it at once, four single additions in
// fp32 (that is across), whatever mode the value is in then, and the rest at once if they fit now.  What is left stays
// pending: the lane comes back in the next iteration of its loop.  Kept short on purpose -- in a wave of 64 some lane
// is here in almost every iteration (9 % of the advances: an image has a binade boundary in its middle), and the wave
// pays for its longest lane (a loop to completion here: 3/4 of the kernel's time).
KBE_HD void axis_catch_up(Axis& ax, int& r, float u, bool subtract, float limit)
{
    if (u == 0.0f) { r = 0; return; }                           // a + 0 = a
    if (ax.e >= 0) {
        const int mag = imax(1, abs(ax.step));
        const int room = ax.step < 0 ? ax.A - (1 << 23) - mag : (1 << 24) - 1 - mag - ax.A;
        const int j = imin(r, (int) ((float) room * rcp_guess((float) mag)) - 1);
        if (j >= 1 && axis_interior(ax.A + j * ax.step, mag)) { ax.A += j * ax.step; r -= j; }      // the test is what counts, j only a guess
    }
    float f = axis_value(ax);
#pragma unroll
    for (int i = 0; i < 4; i++) if (r > 0) { f = subtract ? f - u : f + u; r--; }       // :876-877 / :887-888
    if (f < -1.0f || f > limit) r = 0;                          // outside the image for good: the value no longer matters
    ax = axis_enter(f, u, subtract);
    if (r > 0) axis_jump(ax, r);
}

// ---------------------------------------------------------------------------------------
// the contest of a hole's directions (k_fill_tables, an LDS atomicMin per complete direction)
// ---------------------------------------------------------------------------------------

// the contest's key holds an end's step count in 14 bits: a ray takes at most max(W, H) / 0.707 steps (larger frames
// fill with the other schedules)
constexpr int FILL_MAX_STEPS = (1 << 14) - 1;
KBE_HD bool fill_tables_fit(int W, int H) { return W <= 11000 && H <= 11000; }

// The key of a complete direction: the fp32 length of its span in the high word -- positive floats order like their bits --
// then the direction (the reference keeps the FIRST direction of the shortest length: `best > dd` is strict, common.py:900),
// then the step counts of its two ends, from which the winner's end points are recomputed (advance_exact).
constexpr unsigned long long FILL_NO_ENTRY = ~0ull;
struct FillKey { int d, ka, kb; };
KBE_HD unsigned long long fill_key_pack(float length, int d, int ka, int kb)
{
    return ((unsigned long long) f32_bits(length) << 32) | ((unsigned long long) d << 28) | ((unsigned long long) ka << 14) | (unsigned long long) kb;
}
KBE_HD FillKey fill_key_unpack(unsigned long long key)
{
    return FillKey{ (int) (key >> 28) & 15, (int) (key >> 14) & FILL_MAX_STEPS, (int) key & FILL_MAX_STEPS };
}

// ---------------------------------------------------------------------------------------
// strip tables
// ---------------------------------------------------------------------------------------

// A ray of direction u through a hole p stays within 0.75 pixels of the line through p (positions are
// rounded per axis; the fp32 sums drift by < 0.03 over 1000 steps), so the only valid pixels it can ever meet lie in the
// strip of lines c in [b - 1, b + 2), b = floor(c(p)), c(q) = n . q the coordinate across the direction.  Per direction
// and b, (lo, hi) bound the coordinate t(q) = u . q along the direction over every valid pixel of that strip -- or rather
// over exactly those (strip_bounds: the tiles' boxes first, then the bitmask's rows at either end).  The end walking towards -u meets nothing once lo > t + 1, the end towards +u once hi < t - 1: the
// direction is skipped (common.py:880-885, 891-896) without walking to the image border.  A zoomed-out frame is mostly
// border around a convex patch of valid pixels; outside a convex patch NO direction has valid pixels on both sides.
// Measured on the last frame of the dolly bench (266 k holes inside the box of valid pixels): 1.7 of a hole's 16 directions
// complete, 4.5 pass this test; pixel steps per hole 6811 -> 560 (tests/fill_walk_check.cpp, against brute-force walks: no
// direction that completes is ever skipped).
constexpr float STRIP_MARGIN = 1.0f;
constexpr int STRIP_TILES = 512;                    // the tables are built from the boxes of up to STRIP_TILES tile rows / columns
KBE_HD bool strips_fit(int tiles_x, int tiles_y) { return tiles_x <= STRIP_TILES && tiles_y <= STRIP_TILES; }
KBE_HD int strip_bins(int W, int H) { return W + H + 8; }
// c(q) = -uy x + ux y over the image starts at -(max(0, uy W) + max(0, -ux H)); + 2 keeps b - 1 non-negative
KBE_HD int strip_offset(float ux, float uy, int W, int H)
{
    return (int) ceilf(fmaxf(0.0f, uy * (float) W) + fmaxf(0.0f, -ux * (float) H)) + 2;
}
// pixel (x, y)'s coordinate across direction u and along it, and the line of an across coordinate: the pixel's strip is bin
// strip_line(c) + strip_offset(u)
KBE_HD float strip_across(float ux, float uy, int x, int y) { return ux * (float) y - uy * (float) x; }
KBE_HD float strip_along(float ux, float uy, int x, int y) { return ux * (float) x + uy * (float) y; }
KBE_HD int strip_line(float c) { return (int) floorf(c); }
// The pass test of a hole at t along a direction whose strip is bounded by (lo, hi): valid pixels on one side at most, the
// direction is skipped.  (Phase (1) of k_fill_tables writes these two comparisons out: called from there, this function
// changes the kernel's code.  DESIGN.md section 4.)
KBE_HD bool strip_skip(float lo, float hi, float t) { return lo > t + STRIP_MARGIN || hi < t - STRIP_MARGIN; }
// The end of a ray is past every valid pixel of its strip once its pixel's coordinate along the direction, t = u . q, is more than
// STRIP_MARGIN beyond the strip's bound.  `room`: from the hole to that bound, hi - t_hole for the end towards +u, t_hole - lo for the
// other (-inf: nothing on that side at all).  The pixel k steps on lies within 0.75 of the hole's t -/+ k (a unit direction; rounding per
// axis, < 0.03 of drift), so from k_dead = ceil(room + 2.8) steps on that holds for sure -- one integer comparison per landing instead
// of the coordinate's two conversions, a multiply-add and a comparison (the ray may die two or three steps later than with the
// coordinate itself: it meets nothing there, that is what the bound says)
KBE_HD int strip_k_dead(float room)
{
    return room > (float) FILL_MAX_STEPS ? FILL_MAX_STEPS + 1 : (int) ceilf(fmaxf(room, -2.0f) + STRIP_MARGIN + 1.8f);
}

// (lo, hi) of bin b of direction (ux, uy).  bbox: per tile of TILE_W x TILE_H pixels the box {x, y, z, w} = x0, y0, x1, y1 of its
// valid pixels (inclusive; empty: z < x); mask: the validity bitmask, ceil(W / 32) words per row.
template <int TILE_W, int TILE_H, class Box>
KBE_HD void strip_bounds(int b, const Box* __restrict__ bbox, const uint32_t* __restrict__ mask, int tiles_x, int tiles_y, int W, int H, float ux, float uy, float& lo, float& hi)
{
    const float c0 = (float) (b - strip_offset(ux, uy, W, H)) - STRIP_MARGIN, c1 = c0 + 1.0f + 2.0f * STRIP_MARGIN;
    // Per tile row (tile column for a flat direction) the one to three tiles under the strip, each with the box of its own valid pixels
    // (the tile launch's bbox table), the strip clipped to the box; then the tile whose box reaches farthest towards either end of the
    // strip is looked at ROW BY ROW in the validity bitmask: its valid pixels of the strip give that end's bound, unless another tile's
    // box reaches farther than they do (then that box's reach does: still a superset).  Until round 5: the x-extent of each whole tile
    // ROW (the y-extent of each tile column) -- 4.46 of a late dolly frame's 16 directions per hole passed the test where 1.73
    // complete; the tiles' own boxes alone: 2.47; with the one tile looked at: 2.01; every tile looked at until nothing can improve
    // (exact): 1.91 -- but that walk's chain of dependent loads made k_hole_dist slower than the fill gained (a host prototype on
    // the oracle's masks).  The directions that pass without completing are the expensive ones: they
    // walk to the end of their strip.
    const bool steep = fabsf(uy) >= fabsf(ux);                  // the line crosses every row once: walk the tile rows
    const int n = steep ? tiles_y : tiles_x, m = steep ? tiles_x : tiles_y;
    const float ua = steep ? ux : uy, ub = steep ? uy : ux;     // a = the coordinate along a row (column), b = across
    const float inv = 1.0f / ub;
    const int sa = steep ? TILE_W : TILE_H, sb = steep ? TILE_H : TILE_W;
    const int wpr = (W + 31) >> 5;
    const bool rows_cross = fabsf(uy) >= 1.0e-6f;               // else: a horizontal direction, a strip is whole rows
    const float inv_uy = rows_cross ? 1.0f / uy : 0.0f;
    static_assert(TILE_W == 32 && TILE_H <= 16, "a tile row is one word of the validity bitmask, a tile at most sixteen of them");
    // the strip's extent along a over the rows (columns) b0 .. b1 -- steep: c = -uy x + ux y => x = (ux y - c) / uy; flat: y = (c + uy x) / ux
    const auto along = [&](float b0, float b1, float& a0, float& a1) {
        const float v0 = steep ? (ua * b0 - c0) * inv : (c0 + ua * b0) * inv, v1 = steep ? (ua * b0 - c1) * inv : (c1 + ua * b0) * inv;
        const float v2 = steep ? (ua * b1 - c0) * inv : (c0 + ua * b1) * inv, v3 = steep ? (ua * b1 - c1) * inv : (c1 + ua * b1) * inv;
        a0 = fminf(fminf(v0, v1), fminf(v2, v3)) - 0.01f; a1 = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)) + 0.01f;
    };
    float lo1 = INFINITY, lo2 = INFINITY, hi1 = -INFINITY, hi2 = -INFINITY;        // the farthest and the second farthest reach of a box, either end
    int lo_tile = -1, hi_tile = -1;
    for (int i = 0; i < n; i++) {
        float a0, a1;
        along((float) (i * sb), (float) (i * sb + sb - 1), a0, a1);
        const int j0 = imax((int) floorf(a0 / (float) sa), 0), j1 = imin((int) floorf(a1 / (float) sa), m - 1);
        for (int j = j0; j <= j1; j++) {
            const int tile = steep ? i * tiles_x + j : j * tiles_x + i;
            const Box bb = bbox[tile];
            if (bb.z < bb.x) continue;                          // a tile without a valid pixel
            const float q0 = (float) (steep ? bb.y : bb.x), q1 = (float) (steep ? bb.w : bb.z);        // the box across ...
            float p0, p1;
            along(q0, q1, p0, p1);
            p0 = fmaxf(p0, (float) (steep ? bb.x : bb.y)); p1 = fminf(p1, (float) (steep ? bb.z : bb.w));     // ... and along
            if (p0 > p1) continue;
            // t = ux x + uy y = ua a + ub b over [p0, p1] x [q0, q1]
            const float t0 = ua * p0 + ub * q0, t1 = ua * p0 + ub * q1, t2 = ua * p1 + ub * q0, t3 = ua * p1 + ub * q1;
            const float tmin = fminf(fminf(t0, t1), fminf(t2, t3)), tmax = fmaxf(fmaxf(t0, t1), fmaxf(t2, t3));
            if (tmin < lo1) { lo2 = lo1; lo1 = tmin; lo_tile = tile; } else lo2 = fminf(lo2, tmin);
            if (tmax > hi1) { hi2 = hi1; hi1 = tmax; hi_tile = tile; } else hi2 = fmaxf(hi2, tmax);
        }
    }
    // the valid pixels of the strip in one tile, row by row in the bitmask (the sixteen words requested together): the smallest
    // (`low`) or the largest t among them; none: +inf / -inf
    const auto in_tile = [&](int tile, bool low) -> float {
        float best = low ? INFINITY : -INFINITY;
        if (tile < 0) return best;
        const Box bb = bbox[tile];
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x, x0 = tx * TILE_W;
        uint32_t words[TILE_H];
#pragma unroll
        for (int r = 0; r < TILE_H; r++) words[r] = mask[(size_t) imin(bb.y + r, bb.w) * wpr + tx];
#pragma unroll
        for (int r = 0; r < TILE_H; r++) {
            const int y = bb.y + r;
            if (y > bb.w) continue;
            float xa = -1.0e9f, xb = 1.0e9f;
            if (rows_cross) {
                const float e0 = (ux * (float) y - c0) * inv_uy, e1 = (ux * (float) y - c1) * inv_uy;
                xa = fminf(e0, e1) - 0.01f; xb = fmaxf(e0, e1) + 0.01f;
            } else {
                const float c = ux * (float) y;
                if (c < c0 - 0.01f || c > c1 + 0.01f) continue;
            }
            const int xl = (int) ceilf(fmaxf(xa, (float) bb.x)), xr = (int) floorf(fminf(xb, (float) bb.z));
            if (xl > xr) continue;
            const uint32_t w = words[r] & (0xFFFFFFFFu << (xl - x0)) & (0xFFFFFFFFu >> (31 - (xr - x0)));
            if (!w) continue;
            const float ta = ux * (float) (x0 + __builtin_ctz(w)) + uy * (float) y, tb = ux * (float) (x0 + 31 - __builtin_clz(w)) + uy * (float) y;
            best = low ? fminf(best, fminf(ta, tb)) : fmaxf(best, fmaxf(ta, tb));
        }
        return best;
    };
    lo = fminf(in_tile(lo_tile, true), lo2); hi = fmaxf(in_tile(hi_tile, false), hi2);
}

// ---------------------------------------------------------------------------------------
// jump lengths from the distance tables (k_hole_dist: a pixel's Chebyshev distance D to the nearest valid pixel, capped; a
// block's distance c, in 8 x 8 blocks, to the nearest block with a valid pixel: D >= 8 (c - 1) + 1 for every pixel of it)
// ---------------------------------------------------------------------------------------

// With the nearest valid pixel D away (Chebyshev) from this one, the pixel j steps on is at most j max(|ux|, |uy|) + 1 away
// from this one (the steps; the rounding of both positions; < 0.03 of drift): a hole for sure while j umax + 1.03 < D.  The
// first position to look at is step ceil((D - 1.03) / umax).
#ifndef KBE_FILL_FINE_BELOW
#define KBE_FILL_FINE_BELOW 2           // coarse distances below this ask the fine table as well (longer jumps, one more load)
#endif
KBE_HD float jump_inv_umax(float ux, float uy) { return 0.999999f / fmaxf(fabsf(ux), fabsf(uy)); }
KBE_HD int jump_from_blocks(int c, float inv_umax) { return (int) ceilf((float) (8 * (c - 1)) * inv_umax - 0.03f); }      // D >= 8 (c - 1) + 1
KBE_HD int jump_from_pixels(int dn, float inv_umax) { return (int) ceilf(((float) dn - 1.03f) * inv_umax); }
// the first jump, from the hole itself, is the same for its 16 directions (it is stored once per hole): a step moves at most 1
// pixel per axis and the hole's own position is exact, so the positions in front of step D - 1 are holes for sure
KBE_HD int first_jump_from_blocks(int c) { return 8 * (c - 1); }
KBE_HD int first_jump_from_pixels(int dn) { return imax(1, dn - 1); }

// ---------------------------------------------------------------------------------------
// launch_fill's decisions
// ---------------------------------------------------------------------------------------

#ifndef KBE_FILL_SERIAL_MIN
#define KBE_FILL_SERIAL_MIN 49152       // holes per frame from which one lane per hole beats one half-wave per hole
#endif
#ifndef KBE_FILL_BLOCK
#define KBE_FILL_BLOCK 256
#endif
#ifndef KBE_FILL_MAX_BLOCKS
#define KBE_FILL_MAX_BLOCKS 2048
#endif
#ifndef KBE_FILL_TABLES_BLOCKS
#define KBE_FILL_TABLES_BLOCKS 768      // workgroups of k_fill_tables per frame (3 per CU; with four frames per launch and four lanes: 96.5 us per dolly frame, 2048: 99.5)
#endif
constexpr int DT_W = 64, DT_H = 32;                 // k_hole_dist: the interior of one workgroup, 2 words x 32 rows

// k_fill_holes' `tables` argument says which frames k_fill_tables, launched in front of it, has filled: 0 = none (it was not
// launched), else 1 + min_holes = the frames with at least min_holes holes (min_holes may be 0, hence the + 1); the others are left
// to k_fill_holes
KBE_HD int fill_tables_arg(bool tables, int min_holes) { return tables ? 1 + min_holes : 0; }
KBE_HD bool fill_tables_left(int tables_arg, int n_holes) { return !tables_arg || n_holes < tables_arg - 1; }

struct FillPlan {
    int fill_mode;                      // k_fill_holes' schedule: 0 = by hole count, 1 = one lane per hole, 2 = one half-wave per hole
    bool tables;                        // k_hole_dist and k_fill_tables in front of it
    int min_holes;                      // ... for the frames with at least this many holes
    int use_strips;
    int dist_gx, dist_gy, image_rows;   // k_hole_dist's grid per frame; its block rows from image_rows on build the strip and block tables
    unsigned tables_blocks, fill_blocks;        // k_fill_tables' and k_fill_holes' workgroups per frame
};

// the launches of a fill of W x H frames of tiles_x x tiles_y tiles of TILE_W x TILE_H under `stages` (KBE_STAGE_FILL_*)
template <int TILE_W, int TILE_H>
inline FillPlan fill_plan(int W, int H, int stages, int tiles_x, int tiles_y)
{
    FillPlan P = {};
    P.fill_mode = (stages & KBE_STAGE_FILL_PER_LANE) ? 1 : ((stages & KBE_STAGE_FILL_PER_HALFWAVE) || !(stages & KBE_STAGE_FILL_BY_COUNT) ? 2 : 0);
    const size_t hw = (size_t) W * H;
    const size_t want_fill = hw / 64, max_fill = (size_t) KBE_FILL_MAX_BLOCKS * 256 / KBE_FILL_BLOCK;       // the same number of threads
    P.fill_blocks = (unsigned) (want_fill < max_fill ? (want_fill > 0 ? want_fill : 1) : max_fill);
    P.tables = (stages & KBE_STAGE_FILL_DIST) && (stages & (KBE_STAGE_FILL_PER_LANE | KBE_STAGE_FILL_BY_COUNT)) && fill_tables_fit(W, H);
    if (!P.tables) return P;
    P.min_holes = (stages & KBE_STAGE_FILL_PER_LANE) ? 0 : KBE_FILL_SERIAL_MIN;
    P.use_strips = strips_fit(tiles_x, tiles_y) ? 1 : 0;
    const int gx = (W + DT_W - 1) / DT_W, gy = (H + DT_H - 1) / DT_H;
    const int cw = tiles_x * (TILE_W / 8), ch = tiles_y * (TILE_H / 8);
    const int extra = 16 * ((strip_bins(W, H) + 255) / 256) + ((cw + DT_W - 1) / DT_W) * ((ch + DT_H - 1) / DT_H);
    P.dist_gx = gx; P.dist_gy = gy + (extra + gx - 1) / gx; P.image_rows = gy;
    P.tables_blocks = (unsigned) ((hw + 255) / 256 < KBE_FILL_TABLES_BLOCKS ? (hw + 255) / 256 : KBE_FILL_TABLES_BLOCKS);
    return P;
}


}  // namespace kbe
