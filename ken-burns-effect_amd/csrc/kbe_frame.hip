// kbe_frame.hip -- the per-frame hot path on the resident point cloud (include/kbe.h, "The frame
// loop of process_kenburns"): project + z-splat + bucket -> tile gather -> hole fill.
//
// Design (MI355X).  The reference scatters every point into a global z-buffer (float CAS loop)
// and then into 5 global accumulator planes, 20 float atomics per point (common.py:435-507,
// :586-669).  Measured on gfx950: L2 float atomics retire ~0.2 T/s (95 us per 1024^2 frame for
// the accumulation alone) and LDS float atomics cost ~49 cycles per wave-level ds_add_f32 (a
// tiled LDS-accumulator version kept every CU's LDS pipe busy for ~90 us).  So the scatter is
// turned into a gather:
//   k_project  one thread per point: shift (common.py:104-109), project (:447-484), ONE native
//              atomic umin on the order-preserving key of dblError into the z-buffer (:486-506),
//              and a 16-byte record {ox, oy, dblError, index} appended to the bucket of every
//              32x16 target tile one of its four corners lies in (appends are aggregated per
//              wave: one counter atomic per distinct tile, records stored coalesced);
//   k_tiles    one workgroup per tile: z-buffer tile + halo -> LDS, degrid (:525-568) in LDS,
//              records -> per-pixel linked lists in LDS (bin = north-west corner; one
//              ds_wrxchg per record), then every pixel walks the 4 bins that can reach it,
//              z-tests (:639) and accumulates (:641) in registers, normalises (:686), applies
//              the hole mask (:253), converts to uint8 (:255) and stores coalesced;
//   (kbe_holes.hip)  the hole list (:838-924) filled with an exact branch-and-bound over the 16 directions;
//   (kbe_fused.hip)  the other scatter route: k_frame, one launch on the packed cloud, z-tile in LDS;
//   k_tiles_nc the same tile machinery for render_pointcloud with any channel count (4 channels at a time);
//   kbe_render_video  the whole loop enqueued from C, consecutive frames on several streams ("lanes"); how the finished
//              frames reach the caller's memory is kbe_handoff.hip's.
// The tile machinery in LDS (record lists, degrid, z-tested gather, epilogue) that k_tiles, k_tiles_nc and k_frame
// share, the tile geometry and the per-view scratch are in kbe_tiles.h.
// No accumulator or float render ever exists in HBM and no floating-point atomic is executed.
// What bounds these kernels is instruction issue, not bandwidth: the code below is
// written branch-free where lanes mostly agree and with wave-uniform work kept on the scalar unit.
//
// Numerics are those of oracle/kbe_oracle.c: the z-buffer is bit-exact (min commutes), degrid
// is the out-of-place schedule, accumulation order is bucket order (not point order).
#include <stdlib.h>
#include <string.h>

#include "kbe_cloud.h"
#include "kbe_handoff.h"
#include "kbe_tiles.h"

using namespace kbe;

namespace {

__global__ void k_scratch_init(uint32_t* zkeys, uint32_t* zkeys_b, size_t hw, int* tile_count, int n_tiles, int* hole_count)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x, gtid = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = gtid; i < hw; i += stride) { zkeys[i] = KBE_ZKEY_EMPTY; if (zkeys_b) zkeys_b[i] = KBE_ZKEY_EMPTY; }
    for (size_t i = gtid; i < (size_t) n_tiles; i += stride) { tile_count[i * CNT_STRIDE] = 0; tile_count[i * CNT_STRIDE + 1] = 0; }      // (+ 1: the arrivals at a shared list, kbe_fused.hip)
    if (gtid < (size_t) HOLE_COUNT_INTS) hole_count[gtid] = 0;
}

// k_scratch_init for the sets `stride` bytes apart, one launch (blockIdx.y = the set; the offsets are those of carve())
__global__ void k_scratch_init_sets(char* base, size_t stride, size_t zkeys, size_t zkeys_b, size_t hw, size_t tile_count, int n_tiles, size_t hole_count)
{
    char* const set = base + (size_t) blockIdx.y * stride;
    uint32_t* const za = (uint32_t*) (set + zkeys), * const zb = (uint32_t*) (set + zkeys_b);
    const size_t step = (size_t) gridDim.x * blockDim.x, gtid = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = gtid; i < hw; i += step) { za[i] = KBE_ZKEY_EMPTY; zb[i] = KBE_ZKEY_EMPTY; }
    for (size_t i = gtid; i < (size_t) n_tiles; i += step) { ((int*) (set + tile_count))[i * CNT_STRIDE] = 0; ((int*) (set + tile_count))[i * CNT_STRIDE + 1] = 0; }
    if (gtid < (size_t) HOLE_COUNT_INTS) ((int*) (set + hole_count))[gtid] = 0;
}

// the hole counters / list totals (HOLE_COUNT_INTS ints) of `n` scratch sets `stride` bytes apart
// ... and both banks of their per-tile list counters (`tile_ints` ints at `tile_first` of the first set; blockIdx.y = the set): a
// video that ended in an error after a launch that had placed ahead leaves the counters of one bank standing
__global__ void k_zero_counters(int* first, size_t stride, int n, int* tile_first, size_t tile_ints)
{
    static_assert(HOLE_COUNT_INTS == 8, "k >> 3, k & 7");
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int k = threadIdx.x; k < HOLE_COUNT_INTS * n; k += blockDim.x) ((int*) ((char*) first + (size_t) (k >> 3) * stride))[k & 7] = 0;
    int* const t = (int*) ((char*) tile_first + (size_t) blockIdx.y * stride);
    for (size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x; k < tile_ints; k += (size_t) gridDim.x * blockDim.x) t[k] = 0;
}

// ---------------------------------------------------------------------------------------
// launch 1: project every point once
// ---------------------------------------------------------------------------------------
struct ProjectArgs {
    const float* points;    // [3,N]
    int N;
    int raster_w, raster_n; // hint: the first raster_n points are a row-major raster raster_w wide (0: unknown)
    Camera cam;
    uint32_t* zkeys;
    int* tile_count;
    float4* buckets;
    int tiles_x, tiles_y;
    int* hole_count;
    int dense;              // more than two points per target pixel: pre-reduce the z-splat within the wave
    int buckets_32bit;      // every bucket ends below byte 2^32 of `buckets`
};

// Groups the lanes of a wave by target tile: for a lane that `want`s, `same` is the mask of the
// lanes wanting the same tile and `leader` its lowest lane.  Pure cross-lane work (ballots,
// shuffles), no memory traffic; one loop trip per distinct tile (1-3 for coherent points).
struct TileGroup { unsigned long long same; int leader; };

__device__ __forceinline__ TileGroup group_by_tile(bool want, int tile)
{
    TileGroup g = { 0ull, 0 };
    unsigned long long pending = __ballot(want);
    while (pending) {                                           // wave-uniform
        const int leader = __ffsll((long long) pending) - 1;
        const int t = __builtin_amdgcn_readlane(tile, leader);     // leader is wave-uniform: v_readlane, not an LDS round trip (ds_bpermute)
        const unsigned long long same = __ballot(want && tile == t);
        if (want && tile == t) { g.same = same; g.leader = leader; }
        pending &= ~same;
    }
    return g;
}

// The groups of the east spills follow from the groups of the own tiles: lanes that share an own tile share its
// east neighbour, so a group's spilling lanes are `same & ballot(spills)` and no second grouping loop is needed --
// except for lanes whose own tile is outside the image (corner at -1) but whose east tile is inside.
__device__ __forceinline__ TileGroup east_groups(const TileGroup& own, bool want_own, bool want_east, int east_tile)
{
    const unsigned long long sp = __ballot(want_east);
    TileGroup g = group_by_tile(want_east && !want_own, east_tile);            // normally no lane: the loop does not run
    if (want_east && want_own) {
        g.same = own.same & sp;
        g.leader = __ffsll((long long) g.same) - 1;
    }
    return g;
}

constexpr int UNIT = 64;                // points per wave unit: one per lane (4 per lane needed 98-118 VGPRs, halved the
                                        // occupancy and doubled the time of this kernel; 2 per lane measured 9 % slower)
constexpr int PATCH_ROWS = 2;           // a raster unit is a 32 x 2 patch

// One wave handles units of 64 points, one per lane.  Per unit: load, shift (common.py:104-109), project
// (:447-468), then -- as soon as the image position is known -- the bucket bookkeeping: the point goes to the
// bucket of the tile of its north-west corner (e = 0) and, when that corner sits in a tile's last column (or at
// -1, just outside), also to the east neighbour (e = 1); the lanes of a wave share very few target tiles, so they
// are grouped and one leader per tile bumps the counter for all of them.  A returning global atomic is a ~2 us
// round trip (probe: with the results unused this launch is 3.8 us shorter), so all counter atomics of the round
// are issued back to back and the rest of the point's work -- weights (:472-484), dblError (:470), winner corner
// and the z-splat atomic umin (:486-506) -- is done while they are in flight; only then are the results consumed
// and the 16-byte records stored.  Points whose corner also sits in a tile's last ROW need a second round
// (south, south-east); ~6 % of the waves of a raster.
#ifndef KBE_PROJECT_BLOCK
#define KBE_PROJECT_BLOCK 64        // one wave per workgroup: fits the gaps other lanes' kernels leave (29.7 vs 30.6 us per frame at 256)
#endif
__device__ __forceinline__ void project_body(const ProjectArgs& a)
{
    const int lane = threadIdx.x & 63;
    // wave-uniform values are made scalar explicitly (the unit -> point index arithmetic below then runs on the
    // scalar unit, once per wave, in 32 bits; as vector 64-bit arithmetic it was a sixth of this kernel's instructions)
    const int wave = __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int n_waves = (int) ((gridDim.x * blockDim.x) >> 6);
    const Camera& cam = a.cam;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.hole_count = 0;
    const size_t N = (size_t) a.N;
    // Work units.  Where the cloud is known to start with a row-major raster (the image pixels), a unit is a
    // 32 x 2 patch of it rather than 64 consecutive pixels of a row: its points then fall into one or two target
    // tiles, and a bucket's records reference neighbouring points.  Pure speed hint.
    const unsigned patches_x = (a.raster_w > 0 && a.raster_w % 32 == 0) ? (unsigned) a.raster_w / 32u : 0u;
    const unsigned patch_rows = patches_x ? ((unsigned) a.raster_n / (unsigned) a.raster_w) / PATCH_ROWS : 0u;
    const unsigned n_patches = patches_x * patch_rows;                  // <= N / UNIT
    const unsigned lin0 = n_patches * UNIT;                             // points before lin0 are covered by patches
    const unsigned n_units = n_patches + ((unsigned) a.N - lin0 + UNIT - 1) / UNIT;
    for (unsigned unit = (unsigned) wave; unit < n_units; unit += (unsigned) n_waves) {
        unsigned i;
        if (unit < n_patches) {
            // the patch's first point on the scalar unit; a lane adds its row (0 or raster_w) and column
            const unsigned pyb = unit / patches_x, pxb = unit - pyb * patches_x;
            static_assert(PATCH_ROWS == 2, "a lane's patch row is lane >> 5");
            i = (pyb * PATCH_ROWS * (unsigned) a.raster_w + pxb * 32u) + ((lane >> 5) ? (unsigned) a.raster_w : 0u) + (unsigned) (lane & 31);
        } else {
            i = lin0 + (unit - n_patches) * UNIT + (unsigned) lane;
        }
        bool ok = i < (unsigned) a.N;
        float x = 0.0f, y = 0.0f, z = 0.0f, ox = 0.0f, oy = 0.0f;
        if (ok) {
            const uint32_t off = i << 2;                                // N <= 2^30: a 32-bit byte offset on three uniform bases
            x = *(const float*) ((const char*) a.points + off);
            y = *(const float*) ((const char*) (a.points + N) + off);
            z = *(const float*) ((const char*) (a.points + 2 * N) + off);
            apply_shift(cam, x, y, z);
            ok = project_xy(cam, x, y, z, ox, oy);
        }
        Proj p;
        p.nwx = (int) floorf(ox); p.nwy = (int) floorf(oy);
        ok = ok && ((unsigned) (p.nwx + 1) <= (unsigned) cam.W) & ((unsigned) (p.nwy + 1) <= (unsigned) cam.H);      // touches the image at all: -1 <= nw < size
        const bool spx = ok && ((p.nwx + 1) % TW == 0), spy = ok && ((p.nwy + 1) % TH == 0);
        static_assert((TW & (TW - 1)) == 0 && (TH & (TH - 1)) == 0, "tile sizes are powers of two");
        const int tx0 = p.nwx >> __builtin_ctz(TW), ty0 = p.nwy >> __builtin_ctz(TH);              // floor division: -1 for nw == -1

        // round 0: own tile and east neighbour; the counter atomics go out now
        TileGroup grp[2];
        int tgt[2], base[2];
        bool want[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int tx = tx0 + e;
            want[e] = ok && (e == 0 || spx) && ((unsigned) tx < (unsigned) a.tiles_x) & ((unsigned) ty0 < (unsigned) a.tiles_y);
            tgt[e] = __mul24(ty0, a.tiles_x) + tx;                      // 24-bit multiply: full rate (the 32-bit one is quarter rate)
            base[e] = 0;
        }
        grp[0] = group_by_tile(want[0], tgt[0]);
        grp[1] = east_groups(grp[0], want[0], want[1], tgt[1]);
#pragma unroll
        for (int e = 0; e < 2; e++)
            if (want[e] && lane == grp[e].leader) base[e] = atomicAdd(&a.tile_count[(uint32_t) tgt[e] * CNT_STRIDE], __popcll(grp[e].same));

        // ... and while they are in flight: weights, dblError, winner corner, z-splat
        float err = 0.0f;
        int zidx = -1;
        if (ok) {
            project_weights(ox, oy, p);
            err = project_err_fast(cam, z);
            const int k = winner_corner(p);                             // common.py:486-506
            if (k >= 0) {
                const int cx = p.nwx + (k & 1), cy = p.nwy + (k >> 1);
                if (inside(cx, cy, cam.W, cam.H)) zidx = __mul24(cy, cam.W) + cx;
            }
        }
        if (a.dense) {
            // a cloud denser than the target raster (BASELINE configs[4]: 4 points per pixel): the 2 x 2 source
            // neighbours (lanes ^1, ^32, ^33 of a 32 x 2 patch) mostly splat onto the same pixel and their atomics
            // would serialise on one address (measured: 8x the time per atomic); the lowest lane of those that agree
            // issues one atomic with their minimum
            uint32_t key = zkey_encode(err);
            bool issue = zidx >= 0;
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const int mask = m == 0 ? 1 : (m == 1 ? 32 : 33);
                const int pidx = __shfl_xor(zidx, mask);
                const uint32_t pkey = (uint32_t) __shfl_xor((int) key, mask);
                if (zidx >= 0 && pidx == zidx) {
                    key = min(key, pkey);
                    if ((lane ^ mask) < lane) issue = false;
                }
            }
            if (issue) atomicMin(&a.zkeys[(uint32_t) zidx], key);
        } else if (zidx >= 0) {
            atomicMin(&a.zkeys[(uint32_t) zidx], zkey_encode(err));
        }
        const float4 rec = make_float4(ox, oy, err, __int_as_float((int) i));
        // all buckets within 4 GB (frames up to 4096 x 4096): a 32-bit byte offset from a 24-bit multiply on the
        // uniform base; otherwise 64-bit arithmetic (a quarter-rate multiply-add)
        auto store_record = [&](int tile, int slot) {
            static_assert(BUCKET_STRIDE * 16 < (1 << 24), "the bucket stride in bytes is a 24-bit factor");
            if (a.buckets_32bit) *(float4*) ((char*) a.buckets + (__umul24((uint32_t) tile, (uint32_t) BUCKET_STRIDE * 16u) + ((uint32_t) slot << 4))) = rec;
            else a.buckets[(size_t) tile * BUCKET_STRIDE + slot] = rec;
        };
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int b0 = __shfl(base[e], grp[e].leader);
            if (want[e]) {
                const int slot = b0 + __popcll(grp[e].same & ((1ull << lane) - 1ull));
                if (slot < BUCKET_CAP) store_record(tgt[e], slot);      // beyond: the tile sees count > cap
            }
        }
        // round 1 (rare): south and south-east neighbours
        if (__ballot(spy) != 0ull) {                                    // wave-uniform
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int tx = tx0 + e, ty = ty0 + 1;
                want[e] = spy && (e == 0 || spx) && ((unsigned) tx < (unsigned) a.tiles_x) & ((unsigned) ty < (unsigned) a.tiles_y);
                tgt[e] = __mul24(ty, a.tiles_x) + tx;
                base[e] = 0;
            }
            grp[0] = group_by_tile(want[0], tgt[0]);
            grp[1] = east_groups(grp[0], want[0], want[1], tgt[1]);
#pragma unroll
            for (int e = 0; e < 2; e++)
                if (want[e] && lane == grp[e].leader) base[e] = atomicAdd(&a.tile_count[(uint32_t) tgt[e] * CNT_STRIDE], __popcll(grp[e].same));
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int b0 = __shfl(base[e], grp[e].leader);
                if (want[e]) {
                    const int slot = b0 + __popcll(grp[e].same & ((1ull << lane) - 1ull));
                    if (slot < BUCKET_CAP) store_record(tgt[e], slot);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// launch 2: the tile kernel
// ---------------------------------------------------------------------------------------
struct TileArgs {
    const float* points;    // [3,N]  (only the brute-force path of an overflowing bucket reads it)
    const float* image;     // [3,N]
    const float* depth_in;  // [N]
    int N;
    Camera cam;
    const uint32_t* zkeys;
    const int* tile_count;
    const float4* buckets;
    int tiles_x, tiles_y;
    uint32_t* zkeys_clear;  // optional: the OTHER z-buffer, whose pixels of this tile are reset here (and this tile's bucket counter)
    int* tile_count_clear;
    uint8_t* frame;         // [H,W,3]
    float* depth;           // [H*W]
    uint32_t* mask;         // [H][ceil(W/32)]
    int* holes;
    int* hole_count;
    int4* bbox;
    uint32_t* coarse;
    float* render;          // optional [4,H,W] (unfilled; the fill kernel patches the holes)
    float* existing;        // optional [H*W]
    float* zee;             // optional [H*W] degridded z-buffer
    float* zee_pre;         // optional [H*W] pre-degrid z-buffer
};

__device__ __forceinline__ float4 fetch_rgbd(const TileArgs& a, int id)
{
    // uniform plane bases + one 32-bit byte offset per record (N <= 2^30): the loads take the scalar-base form and
    // the lane computes a single shift instead of four 64-bit address additions
    const uint32_t off = (uint32_t) id << 2;
    const char* r = (const char*) a.image;
    const char* g = (const char*) (a.image + (size_t) a.N);
    const char* b = (const char*) (a.image + 2 * (size_t) a.N);
    const char* d = (const char*) a.depth_in;
    return make_float4(*(const float*) (r + off), *(const float*) (g + off), *(const float*) (b + off), *(const float*) (d + off));
}

__device__ __forceinline__ void tiles_body(const TileArgs& a)
{
    __shared__ TileLds L;

    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * TW, y0 = ty * TH;
    const int W = a.cam.W, H = a.cam.H;

    // The launch is latency-bound, so the loads are ordered by what depends on them: the bucket count and this
    // thread's share of the first REC_CAP records first (the colour fetch needs the point indices in them),
    // then its share of the z-buffer tile; the colour loads are issued as soon as the records are in and fly
    // during the z-buffer decode, the first barrier and the degrid.  None of these loads sits under a branch:
    // the compiler's wait-count bookkeeping is per program point, and a load that MAY have been issued makes
    // every later wait on an older load a wait for everything (measured: the colour loads were waited for
    // in front of the degrid instead of behind it).
    const int count = a.tile_count[tile * CNT_STRIDE];
    const bool bucketed = count <= BUCKET_CAP;
    const float4* B = a.buckets + (size_t) tile * BUCKET_STRIDE;
    constexpr int ZPER = (KH * KW + TILE_THREADS - 1) / TILE_THREADS;
    constexpr int PER = (REC_CAP + TILE_THREADS - 1) / TILE_THREADS;
    float4 rr[PER], cc[PER];
    // the first REC_CAP records are loaded WITHOUT waiting for the count (the bucket is at least that
    // large, so the addresses are valid; slots past the count hold stale records and are masked below)
    static_assert(BUCKET_CAP >= ((REC_CAP + TILE_THREADS - 1) / TILE_THREADS) * TILE_THREADS, "speculative bucket loads stay in bounds");
#pragma unroll
    for (int u = 0; u < PER; u++) rr[u] = B[tid + u * TILE_THREADS];
    uint32_t zk[ZPER];
    bool zin[ZPER];
#pragma unroll
    for (int u = 0; u < ZPER; u++) {
        const int i = tid + u * TILE_THREADS;
        const int py = i / KW, pxl = i - py * KW;
        const int xr = x0 - 1 + pxl, yr = y0 - 1 + py;
        zin[u] = inside(xr, yr, W, H);
        const int x = min(max(xr, 0), W - 1), y = min(max(yr, 0), H - 1);       // clamped: always a valid address
        // W * H < 2^31 / 4: a 32-bit byte offset on the uniform base
        // (24-bit multiply: full rate, the 32-bit one is quarter rate; y, W < 2^24)
        zk[u] = *(const uint32_t*) ((const char*) a.zkeys + ((__umul24((uint32_t) y, (uint32_t) W) + (uint32_t) x) << 2));
    }
    lds_reset_heads(L, tid);
    if (tid == 0) {
        L.nrec = 0;
        lds_dummy_record(L);
    }
    // colours of the records (slots past the count: point 0, discarded later; the host never passes a NULL cloud)
    const int n0 = bucketed ? min(REC_CAP, count) : 0;
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int i = tid + u * TILE_THREADS;
        cc[u] = fetch_rgbd(a, i < n0 ? __float_as_int(rr[u].w) : 0);
    }
    bool band = true;
#pragma unroll
    for (int u = 0; u < ZPER; u++) {
        const int i = tid + u * TILE_THREADS;
        if (i < KH * KW) {
            const float z = zkey_decode(zin[u] ? zk[u] : KBE_ZKEY_EMPTY);       // common.py:430 outside
            L.zpre[i] = z;
            band = band && degrid_fast_ok(z);
        }
    }
    {
        const unsigned long long odd = __ballot(!band);
        if (lane == 0) L.odd_z[tid >> 6] = odd != 0ull;
    }
    __syncthreads();
    // one decision per tile: every z of tile + halo in [2^19, 1e6] (any scene whose points are farther than
    // F*B/475712 from the camera) -> fp32-only, branch-free degrid and z test
    const bool fast = lds_tile_is_fast(L);
    tile_degrid(a, L, tid, x0, y0, fast);

    PixAcc acc[PIX_PER_THREAD];
#pragma unroll
    for (int m = 0; m < PIX_PER_THREAD; m++) { acc[m].rg = (f2) (0.0f); acc[m].bd = (f2) (0.0f); acc[m].w = 0.0f; }

    if (bucketed) {
        // the normal path: the tile's records, REC_CAP at a time (one round unless points pile up)
        for (int r0 = 0; r0 == 0 || r0 < count; r0 += REC_CAP) {
            const int n = min(REC_CAP, count - r0);
            if (r0 > 0) {
                __syncthreads();                                // the previous round's gather is done with the lists
                lds_reset_heads(L, tid);
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    rr[u] = i < n ? B[r0 + i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    cc[u] = i < n ? fetch_rgbd(a, __float_as_int(rr[u].w)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
                __syncthreads();
            }
            {
                // all of this thread's list exchanges first, then the records with the links they returned (one after
                // the other each exchange was an LDS round trip in front of the next)
                int nxt[PER];
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    nxt[u] = REC_NULL;
                    if (i < n) {
                        const int bx = (int) floorf(rr[u].x) - (x0 - 1), by = (int) floorf(rr[u].y) - (y0 - 1);
                        L.rgbd[i] = cc[u];
                        nxt[u] = atomicExch(&L.head[__mul24(by, BW) + bx], i << 4);
                    }
                }
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    if (i < n) L.rec[i] = make_float4(rr[u].x, rr[u].y, rr[u].z, __int_as_float(nxt[u]));
                }
            }
            __syncthreads();
            if (fast) gather<true>(a, L, tid, x0, y0, acc);
            else gather<false>(a, L, tid, x0, y0, acc);
        }
        // no barrier here: what follows stages its bytes and per-wave partial results in the z-buffer area, dead since
        // the barrier in front of the gather, so a wave that is done resolves its pixels while others still walk
    } else {
        // the bucket overflowed (an extreme pile-up of points on this tile): re-derive the tile's
        // records from the whole cloud, REC_CAP at a time.  Slow, but any cloud renders correctly.
        __syncthreads();
        const int n_round = (a.N + TILE_THREADS - 1) / TILE_THREADS * TILE_THREADS;
        for (int i0 = 0; i0 < n_round; i0 += TILE_THREADS) {
            const int i = i0 + tid;
            bool ok = i < a.N;
            float ox = 0.0f, oy = 0.0f, z = 0.0f;
            if (ok) {
                float x = a.points[i], y = a.points[(size_t) a.N + i];
                z = a.points[2 * (size_t) a.N + i];
                apply_shift(a.cam, x, y, z);
                ok = project_xy(a.cam, x, y, z, ox, oy);
            }
            if (ok) {
                const int bx = (int) floorf(ox) - (x0 - 1), by = (int) floorf(oy) - (y0 - 1);
                ok = (bx >= 0) & (bx < BW) & (by >= 0) & (by < BH);
            }
            const unsigned long long m = __ballot(ok);
            if (m) {
                int base = 0;
                const int leader = __ffsll((long long) m) - 1;
                if (lane == leader) base = atomicAdd(&L.nrec, __popcll(m));
                base = __shfl(base, leader);
                if (ok) lds_insert(L, base + __popcll(m & ((1ull << lane) - 1ull)), ox, oy, project_err(a.cam, z), fetch_rgbd(a, i), x0, y0);
            }
            __syncthreads();
            if (L.nrec + TILE_THREADS > REC_CAP || i0 + TILE_THREADS >= n_round) {      // uniform
                gather<false>(a, L, tid, x0, y0, acc);
                __syncthreads();
                lds_reset_heads(L, tid);
                if (tid == 0) L.nrec = 0;
                __syncthreads();
            }
        }
    }

    tile_epilogue(a, L, acc, tile, x0, y0);
    // Consecutive frames of a video alternate between two z-buffers: this launch leaves the OTHER one empty for the next
    // frame's projection (a tile's pixels of the buffer in use are still being read by its neighbours' halos, so a launch
    // cannot clear its own), and its own bucket counter (nobody else reads it).  That takes the z-buffer / bucket reset
    // -- a launch of its own riding in k_fill_holes for a frame rendered alone -- out of the scatter.
    if (a.zkeys_clear) {
        if (tid == 0) a.tile_count_clear[tile * CNT_STRIDE] = 0;
#pragma unroll
        for (int m = 0; m < PIX_PER_THREAD; m++) {
            const int q = tid + m * TILE_THREADS;
            const int ly = q / TW, lx = q - ly * TW;
            if (x0 + lx < W && y0 + ly < H) a.zkeys_clear[__umul24((uint32_t) (y0 + ly), (uint32_t) W) + (uint32_t) (x0 + lx)] = KBE_ZKEY_EMPTY;
        }
    }
}

// Both launches of the bucket route take up to KBE_SCATTER_JOBS frames (blockIdx.y = the frame; same cloud, same frame
// size, each frame with its own camera and scratch set).  Frames are independent, and a launch on its own is bound by
// its ramp and its latencies, not by the chip: k_project issues for 7 us of its 14, k_tiles for 8 of its 19.5.  Several
// frames per launch fill those gaps inside ONE stream (the video loop's lanes do the same across streams, but HIP maps
// a process's streams onto four hardware queues).
constexpr int KBE_SCATTER_JOBS = KBE_FILL_JOBS;
struct ProjectJobs { ProjectArgs a[KBE_SCATTER_JOBS]; };
struct TileJobs { TileArgs a[KBE_SCATTER_JOBS]; };

__global__ void __launch_bounds__(KBE_PROJECT_BLOCK) k_project(ProjectArgs a)
{
    project_body(a);
}

__global__ void __launch_bounds__(TILE_THREADS) __attribute__((KBE_TILE_ATTR)) k_tiles(TileArgs a)
{
    tiles_body(a);
}

// ... and the forms that take a group of frames (a frame on its own keeps the launches above: their arguments sit in the
// kernel-argument registers, while a group's are indexed by blockIdx.y and loaded by every wave -- 33.5 vs 34.8 us per frame
// for the scatter of a single frame)
__global__ void __launch_bounds__(KBE_PROJECT_BLOCK) k_project_group(ProjectJobs jobs)
{
    project_body(jobs.a[blockIdx.y]);
}

__global__ void __launch_bounds__(TILE_THREADS) __attribute__((KBE_TILE_ATTR)) k_tiles_group(TileJobs jobs)
{
    tiles_body(jobs.a[blockIdx.y]);
}

// ---------------------------------------------------------------------------------------
// render_pointcloud for ANY channel count on the same machinery (the 68-channel forward warp of the inpaint
// set-up, pointcloud_inpainting.py:201: image, disparity and 64 context features): k_project fills the z-buffer
// and the buckets exactly as for a frame; this kernel degrids the tile once and then takes the data four
// channels at a time -- per chunk the records are threaded into the per-pixel lists again with their four values
// (the lists cost little next to the walk), every pixel walks its bins and the chunk leaves normalised
// (common.py:686).  No accumulator in HBM, no floating-point atomic; 20x faster than the global-atomic
// formulation at 68 channels (0.1 vs 2.2 ms at 1024^2).
// ---------------------------------------------------------------------------------------
struct TileNcArgs {
    const float* points;    // [3,N]  (only the brute-force path of an overflowing bucket reads it)
    const float* data;      // [C,N]
    int N, C;
    Camera cam;
    const uint32_t* zkeys;
    const int* tile_count;
    const float4* buckets;
    int tiles_x, tiles_y;
    float* render;          // [C,H,W] normalised
    float* existing;        // [H*W] weight sum
};

__device__ __forceinline__ float4 fetch_chunk(const TileNcArgs& a, int id, int c0)
{
    const size_t N = (size_t) a.N;
    const float* D = a.data + (size_t) c0 * N + id;
    float4 v;
    v.x = D[0];
    v.y = c0 + 1 < a.C ? D[N] : 0.0f;
    v.z = c0 + 2 < a.C ? D[2 * N] : 0.0f;
    v.w = c0 + 3 < a.C ? D[3 * N] : 0.0f;
    return v;
}

__global__ void __launch_bounds__(TILE_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) k_tiles_nc(TileNcArgs a)
{
    __shared__ TileLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * TW, y0 = ty * TH;
    const int W = a.cam.W, H = a.cam.H;
    const size_t HW = (size_t) W * H;
    const int count = a.tile_count[tile * CNT_STRIDE];
    const bool bucketed = count <= BUCKET_CAP;
    const float4* B = a.buckets + (size_t) tile * BUCKET_STRIDE;
    constexpr int PER = (REC_CAP + TILE_THREADS - 1) / TILE_THREADS;

    // z tile + halo -> LDS, one decision per tile (see k_tiles), degrid
    bool band = true;
    for (int i = tid; i < KH * KW; i += TILE_THREADS) {
        const int py = i / KW, pxl = i - py * KW;
        const int x = x0 - 1 + pxl, y = y0 - 1 + py;
        const float z = zkey_decode(inside(x, y, W, H) ? a.zkeys[(size_t) y * W + x] : KBE_ZKEY_EMPTY);     // common.py:430 outside
        L.zpre[i] = z;
        band = band && degrid_fast_ok(z);
    }
    {
        const unsigned long long odd = __ballot(!band);
        if (lane == 0) L.odd_z[tid >> 6] = odd != 0ull;
    }
    if (tid == 0) lds_dummy_record(L);
    __syncthreads();
    const bool fast = lds_tile_is_fast(L);
    for (int i = tid; i < TH * TW; i += TILE_THREADS) {
        const int ly = i / TW, lx = i - ly * TW;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        auto at = [&](int xx, int yy) { return L.zpre[(yy - y0 + 1) * KW + (xx - x0 + 1)]; };
        L.zee[i] = degrid_pixel(x, y, W, H, at);
    }

    for (int c0 = 0; c0 < a.C; c0 += 4) {
        PixAcc acc[PIX_PER_THREAD];
#pragma unroll
        for (int m = 0; m < PIX_PER_THREAD; m++) { acc[m].rg = (f2) (0.0f); acc[m].bd = (f2) (0.0f); acc[m].w = 0.0f; }
        if (bucketed) {
            for (int r0 = 0; r0 == 0 || r0 < count; r0 += REC_CAP) {
                const int n = min(REC_CAP, count - r0);
                float4 rr[PER], cc[PER];
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    rr[u] = B[min(r0 + i, BUCKET_CAP - 1)];                // unconditional (clamped) loads: see k_tiles
                }
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    cc[u] = fetch_chunk(a, i < n ? __float_as_int(rr[u].w) : 0, c0);
                }
                __syncthreads();                                        // zee written / the previous gather is done with the lists
                lds_reset_heads(L, tid);
                __syncthreads();
#pragma unroll
                for (int u = 0; u < PER; u++) {
                    const int i = tid + u * TILE_THREADS;
                    if (i < n) lds_insert(L, i, rr[u].x, rr[u].y, rr[u].z, cc[u], x0, y0);
                }
                __syncthreads();
                if (fast) gather<true>(a, L, tid, x0, y0, acc);
                else gather<false>(a, L, tid, x0, y0, acc);
            }
        } else {
            // the bucket overflowed (an extreme pile-up of points on this tile): re-derive the tile's records from the
            // whole cloud, REC_CAP at a time.  Slow, but any cloud renders correctly.
            __syncthreads();
            lds_reset_heads(L, tid);
            if (tid == 0) L.nrec = 0;
            __syncthreads();
            const int n_round = (a.N + TILE_THREADS - 1) / TILE_THREADS * TILE_THREADS;
            for (int i0 = 0; i0 < n_round; i0 += TILE_THREADS) {
                const int i = i0 + tid;
                bool ok = i < a.N;
                float ox = 0.0f, oy = 0.0f, z = 0.0f;
                if (ok) {
                    float x = a.points[i], y = a.points[(size_t) a.N + i];
                    z = a.points[2 * (size_t) a.N + i];
                    apply_shift(a.cam, x, y, z);
                    ok = project_xy(a.cam, x, y, z, ox, oy);
                }
                if (ok) {
                    const int bx = (int) floorf(ox) - (x0 - 1), by = (int) floorf(oy) - (y0 - 1);
                    ok = (bx >= 0) & (bx < BW) & (by >= 0) & (by < BH);
                }
                const unsigned long long m = __ballot(ok);
                if (m) {
                    int base = 0;
                    const int leader = __ffsll((long long) m) - 1;
                    if (lane == leader) base = atomicAdd(&L.nrec, __popcll(m));
                    base = __builtin_amdgcn_readlane(base, leader);
                    if (ok) lds_insert(L, base + __popcll(m & ((1ull << lane) - 1ull)), ox, oy, project_err(a.cam, z), fetch_chunk(a, i, c0), x0, y0);
                }
                __syncthreads();
                if (L.nrec + TILE_THREADS > REC_CAP || i0 + TILE_THREADS >= n_round) {      // uniform
                    gather<false>(a, L, tid, x0, y0, acc);
                    __syncthreads();
                    lds_reset_heads(L, tid);
                    if (tid == 0) L.nrec = 0;
                    __syncthreads();
                }
            }
        }
        // the chunk leaves normalised (common.py:686); the weight sum with the first chunk
#pragma unroll
        for (int m = 0; m < PIX_PER_THREAD; m++) {
            const int q = tid + m * TILE_THREADS;
            const int ly = q / TW, lx = q - ly * TW;
            const int x = x0 + lx, y = y0 + ly;
            if (x >= W || y >= H) continue;
            const size_t o = (size_t) y * W + x;
            const float den = acc[m].w + 0.0000001f;
            a.render[(size_t) c0 * HW + o] = acc[m].rg.x / den;
            if (c0 + 1 < a.C) a.render[(size_t) (c0 + 1) * HW + o] = acc[m].rg.y / den;
            if (c0 + 2 < a.C) a.render[(size_t) (c0 + 2) * HW + o] = acc[m].bd.x / den;
            if (c0 + 3 < a.C) a.render[(size_t) (c0 + 3) * HW + o] = acc[m].bd.y / den;
            if (c0 == 0) a.existing[o] = acc[m].w;
        }
    }
}

}  // namespace

extern "C" {

size_t kbe_frame_scratch_bytes(int W, int H, int N)
{
    return (W <= 0 || H <= 0 || N < 0) ? 0 : scratch_set_bytes(W, H, N);
}

size_t kbe_video_scratch_stride(int W, int H, int N)
{
    return (W <= 0 || H <= 0 || N < 0) ? 0 : ((scratch_set_bytes(W, H, N) + 255) & ~(size_t) 255);
}

size_t kbe_video_stage_bytes(int W, int H, int lanes, int batch)
{
    if (W <= 0 || H <= 0 || lanes < 1) return 0;
    return stage_layout(W, H, lanes, batch, KBE_FRAME_JOBS).total;      // frames + the hand-off's turn counter (kbe_video_plan.h)
}

int kbe_frame_scratch_init(void* scratch, int W, int H, kbe_stream_t stream)
{
    KBE_REQUIRE(scratch && W > 0 && H > 0 && ((uintptr_t) scratch & 15) == 0, "kbe_frame_scratch_init: bad arguments");
    const Scratch sc = carve(scratch, W, H);
    // (both banks of counters: 4 * n_tiles * CNT_STRIDE bytes is a multiple of 16, so the banks are contiguous)
    hipLaunchKernelGGL(k_scratch_init, dim3(1024), dim3(256), 0, (hipStream_t) stream, sc.zkeys, sc.zkeys_b, (size_t) W * H, sc.tile_count,
                       2 * sc.tiles_x * sc.tiles_y, sc.hole_count);
    return launched("kbe_frame_scratch_init");
}

int kbe_frame_scratch_init_sets(void* scratch, size_t stride, int n, int W, int H, kbe_stream_t stream)
{
    KBE_REQUIRE(scratch && n > 0 && n <= 65535 && W > 0 && H > 0 && ((uintptr_t) scratch & 15) == 0 && (stride & 15) == 0 && stride >= scratch_bytes(W, H),
                "kbe_frame_scratch_init_sets: bad arguments");
    const Scratch sc = carve(scratch, W, H);
    auto off = [&](const void* p) { return (size_t) ((const char*) p - (const char*) scratch); };
    hipLaunchKernelGGL(k_scratch_init_sets, dim3(256, n), dim3(256), 0, (hipStream_t) stream, (char*) scratch, stride, off(sc.zkeys), off(sc.zkeys_b), (size_t) W * H,
                       off(sc.tile_count), 2 * sc.tiles_x * sc.tiles_y, off(sc.hole_count));
    return launched("kbe_frame_scratch_init_sets");
}

}  // extern "C"

namespace {
// the frame sizes the routes take (include/kbe.h): pixel offsets in 32 bits, coordinates through 24-bit multiplies -- SIGNED ones
// among them (k_project's z-splat index, __mul24(cy, cam.W)), which read a factor of 2^23 or more as negative
bool frame_size_ok(int W, int H) { return W > 0 && H > 0 && (size_t) W * H <= (1u << 30) && W < (1 << 23) && H < (1 << 23); }

// the scratch sets of a group of `n` frames (and their frames and turns, where given): non-null, 16-byte aligned, turns >= 0, no set
// used twice.  KBE_OK, or KBE_E_INVALID with `bad` or `twice` as the error.
int check_sets(int n, void* const* sets, uint8_t* const* frames, const int* turns, const char* bad, const char* twice)
{
    for (int k = 0; k < n; k++) {
        KBE_REQUIRE(sets[k] && (!frames || frames[k]) && ((uintptr_t) sets[k] & 15) == 0 && (!turns || turns[k] >= 0), bad);
        for (int j = 0; j < k; j++) KBE_REQUIRE(sets[j] != sets[k], twice);
    }
    return KBE_OK;
}

// include/kbe.h's `fill_rect` {x0, y0, x1, y1} (NULL: the whole frame)
FillRect fill_rect_of(const int* r, int W, int H) { return r ? FillRect{ r[0], r[1], r[2], r[3] } : FillRect{ 0, 0, W - 1, H - 1 }; }

// launched() with the error named "<label>/<step>"
int launched_as(const char* label, const char* step)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return KBE_OK;
    char what[96];
    snprintf(what, sizeof(what), "%s/%s", label, step);
    return fail(KBE_E_LAUNCH, what, e);
}

// one frame of a group: its camera, its scratch set, where it goes, which of the set's z-buffers it uses (KBE_STAGE_ZBUF_*)
struct FrameJob {
    double focal;
    const float* shift3;
    void* scratch;
    uint8_t* frame_u8;
    float* render_f32; float* existing_f32; float* zee_f32; float* zee_pre_f32;
    int zflags;
};

// the launches of `n` frames of the same cloud and size, each launch taking all n frames (bucket route)
int render_jobs(const float* points, const float* image, const float* depth, int N, int W, int H, double baseline, int n, const FrameJob* jobs,
                int stages, const int* fill_rect, int raster_w, int raster_n, hipStream_t s)
{
    static const FillDirs dirs = make_fill_dirs();
    ProjectJobs pj;
    TileJobs tj;
    FillTarget targets[KBE_SCATTER_JOBS];
    int n_tiles = 0, rc = KBE_OK;
    for (int k = 0; k < KBE_SCATTER_JOBS; k++) {
        const FrameJob& job = jobs[k < n ? k : 0];
        const Scratch sc = carve(job.scratch, W, H);
        const Camera cam = make_camera(W, H, job.focal, baseline, job.shift3);
        n_tiles = sc.tiles_x * sc.tiles_y;
        // which z-buffer this frame splats into, and whether its tile launch clears the other one (include/kbe.h)
        const bool alternate = (job.zflags & (KBE_STAGE_ZBUF_A | KBE_STAGE_ZBUF_B)) != 0;
        uint32_t* const zk_use = (job.zflags & KBE_STAGE_ZBUF_B) ? sc.zkeys_b : sc.zkeys;
        uint32_t* const zk_other = (job.zflags & KBE_STAGE_ZBUF_B) ? sc.zkeys : sc.zkeys_b;
        ProjectArgs& p = pj.a[k];
        p.points = points; p.N = N; p.cam = cam; p.zkeys = zk_use; p.tile_count = sc.tile_count; p.buckets = sc.buckets;
        p.tiles_x = sc.tiles_x; p.tiles_y = sc.tiles_y; p.hole_count = sc.hole_count;
        p.raster_w = 0; p.raster_n = 0;
        p.dense = (size_t) N > 2 * (size_t) W * H;
        p.buckets_32bit = (size_t) n_tiles * BUCKET_STRIDE * sizeof(float4) <= ((size_t) 1 << 32);
        if (raster_w > 0 && raster_n >= raster_w && raster_n <= N && raster_n % raster_w == 0) { p.raster_w = raster_w; p.raster_n = raster_n; }
        TileArgs& a = tj.a[k];
        a.points = points; a.image = image; a.depth_in = depth; a.N = N; a.cam = cam;
        if (N == 0) a.points = a.image = a.depth_in = (const float*) sc.zkeys;     // never dereferenced for a record, but never NULL
        a.zkeys = zk_use; a.tile_count = sc.tile_count; a.buckets = sc.buckets; a.tiles_x = sc.tiles_x; a.tiles_y = sc.tiles_y;
        a.zkeys_clear = alternate ? zk_other : nullptr; a.tile_count_clear = sc.tile_count;
        a.frame = job.frame_u8; a.depth = sc.depth; a.mask = sc.mask; a.holes = sc.holes; a.hole_count = sc.hole_count; a.bbox = sc.bbox; a.coarse = sc.coarse;
        a.render = job.render_f32; a.existing = job.existing_f32; a.zee = job.zee_f32; a.zee_pre = job.zee_pre_f32;
        targets[k] = FillTarget{ sc, sc.hole_count, job.frame_u8, job.render_f32, alternate ? 0 : 1, nullptr };
    }
    if (stages & KBE_STAGE_PROJECT) {
#ifndef KBE_PROJECT_MAX_BLOCKS
#define KBE_PROJECT_MAX_BLOCKS 1000000
#endif
        unsigned blocks = N > 0 ? blocks_for((size_t) N, KBE_PROJECT_BLOCK) + 2 : 1;
        if (blocks > KBE_PROJECT_MAX_BLOCKS) blocks = KBE_PROJECT_MAX_BLOCKS;
        if (n == 1) hipLaunchKernelGGL(k_project, dim3(blocks), dim3(KBE_PROJECT_BLOCK), 0, s, pj.a[0]);
        else hipLaunchKernelGGL(k_project_group, dim3(blocks, n), dim3(KBE_PROJECT_BLOCK), 0, s, pj);
        if ((rc = launched("kbe_render_frame/project"))) return rc;
    }
    if (stages & KBE_STAGE_TILES) {
        if (n == 1) hipLaunchKernelGGL(k_tiles, dim3(n_tiles), dim3(TILE_THREADS), 0, s, tj.a[0]);
        else hipLaunchKernelGGL(k_tiles_group, dim3(n_tiles, n), dim3(TILE_THREADS), 0, s, tj);
        if ((rc = launched("kbe_render_frame/tiles"))) return rc;
    }
    if (stages & KBE_STAGE_FILL) {
        launch_fill(s, n, targets, W, H, stages, dirs, fill_rect_of(fill_rect, W, H), n_tiles);
        rc = launched("kbe_render_frame/fill");
    }
    return rc;
}

// frame `frame` of the fused route on the scratch set at `set`: its camera, and which of the set's counters and banks it uses
FusedTarget fused_target(void* set, int W, int H, double focal, double baseline, const float* shift3, int parity, uint8_t* frame, int turn)
{
    return FusedTarget{ make_camera(W, H, focal, baseline, shift3), carve(set, W, H), scratch_place(set, W, H), parity, frame, nullptr, nullptr, nullptr, nullptr, turn };
}

// The counter resets of the fused route, each caller's own (kbe_render_video zeroes every set's once per call: k_zero_counters).
// A frame on its own: the caller keeps no frame parity, so the set's hole counters and list totals (and the binning launch's flags
// behind them) are zeroed in front of the launch.
int zero_hole_count(const Scratch& sc, hipStream_t s, const char* what)
{
    const hipError_t e = hipMemsetAsync(sc.hole_count, 0, HOLE_COUNT_INTS * sizeof(int), s);
    return e == hipSuccess ? KBE_OK : fail(KBE_E_LAUNCH, what, e);
}
// A set's first turn in a sequence that places ahead: the same, and BOTH banks of its per-tile list counters -- a sequence that was
// abandoned (an error return, a caller that stopped after a launch that placed ahead) leaves the counters of the bank it placed into
// standing, and placements appended behind stale counts list sub-blocks twice.
int start_set(const Scratch& sc, hipStream_t s, const char* what)
{
    if (int rc = zero_hole_count(sc, s, what)) return rc;
    const hipError_t e = hipMemsetAsync(sc.tile_count, 0, 2 * align16(4 * (size_t) sc.tiles_x * sc.tiles_y * CNT_STRIDE), s);
    return e == hipSuccess ? KBE_OK : fail(KBE_E_LAUNCH, what, e);
}

// the launches of `n` frames of the packed cloud (fused route): the scatter takes all n frames -- and makes the placements of the
// `n_next` frames of `next` when asked -- the fill KBE_FILL_JOBS at a time.  The counter resets in front are the callers' (they differ);
// `label` names the errors.
int render_fused(hipStream_t s, const void* packed, int N, double cloud_focal, int n, const FusedTarget* now, bool placed, int n_next,
                 const FusedTarget* next, int stages, int build, const FillRect& rect, double near_depth, const char* label)
{
    static const FillDirs dirs = make_fill_dirs();
    if (stages & KBE_STAGE_TILES) {
        launch_frames_fused(s, n, packed, N, cloud_focal, now, placed, n_next, next, build, near_depth);
        if (int rc = launched_as(label, "scatter")) return rc;
    }
    if (!(stages & KBE_STAGE_FILL)) return KBE_OK;
    // a frame counts its holes in the counter of its parity (-1: counter 0) and, with a parity, zeroes the other one for its set's next frame
    FillTarget targets[KBE_FRAME_JOBS];
    for (int k = 0; k < n; k++) {
        const FusedTarget& t = now[k];
        targets[k] = FillTarget{ t.sc, t.sc.hole_count + (t.parity == 1), t.frame_u8, t.render_f32, 0, t.parity >= 0 ? t.sc.hole_count + (t.parity != 1) : nullptr };
    }
    const int W = now[0].cam.W, H = now[0].cam.H;
    for (int k0 = 0; k0 < n; k0 += KBE_FILL_JOBS)
        launch_fill(s, n - k0 < KBE_FILL_JOBS ? n - k0 : KBE_FILL_JOBS, targets + k0, W, H, stages, dirs, rect, now[0].sc.tiles_x * now[0].sc.tiles_y);
    return launched_as(label, "fill");
}
}  // namespace

extern "C" {

int kbe_render_frame_stages(const float* points, const float* image, const float* depth, int N, int W, int H, double focal,
                            double baseline, const float* shift3, void* scratch, uint8_t* frame_u8, float* render_f32,
                            float* existing_f32, float* zee_f32, float* zee_pre_f32, int stages, const int* fill_rect,
                            int raster_w, int raster_n, kbe_stream_t stream)
{
    KBE_REQUIRE(scratch && frame_u8 && N >= 0 && N <= (1 << 30) && frame_size_ok(W, H) && ((uintptr_t) scratch & 15) == 0, "kbe_render_frame: bad arguments");
    KBE_REQUIRE(N == 0 || (points && image && depth), "kbe_render_frame: cloud pointers are NULL");
    const FrameJob job = { focal, shift3, scratch, frame_u8, render_f32, existing_f32, zee_f32, zee_pre_f32, stages & (KBE_STAGE_ZBUF_A | KBE_STAGE_ZBUF_B) };
    return render_jobs(points, image, depth, N, W, H, baseline, 1, &job, stages, fill_rect, raster_w, raster_n, (hipStream_t) stream);
}

int kbe_render_frame_group(const float* points, const float* image, const float* depth, int N, int W, int H, double baseline, int n_frames,
                           const double* focals, const float* shifts, void* const* scratch, uint8_t* const* frames_u8, const int* zbuf_flags,
                           int stages, const int* fill_rect, int raster_w, int raster_n, kbe_stream_t stream)
{
    KBE_REQUIRE(n_frames >= 1 && n_frames <= KBE_SCATTER_JOBS && focals && shifts && scratch && frames_u8 && N >= 0 && N <= (1 << 30) && frame_size_ok(W, H),
                "kbe_render_frame_group: bad arguments");
    KBE_REQUIRE(N == 0 || (points && image && depth), "kbe_render_frame_group: cloud pointers are NULL");
    if (int rc = check_sets(n_frames, scratch, frames_u8, nullptr, "kbe_render_frame_group: bad scratch / frame pointer",
                            "kbe_render_frame_group: the frames of a group need scratch sets of their own"))
        return rc;
    FrameJob jobs[KBE_SCATTER_JOBS];
    for (int k = 0; k < n_frames; k++)
        jobs[k] = FrameJob{ focals[k], shifts + 3 * (size_t) k, scratch[k], frames_u8[k], nullptr, nullptr, nullptr, nullptr,
                            zbuf_flags ? zbuf_flags[k] & (KBE_STAGE_ZBUF_A | KBE_STAGE_ZBUF_B) : 0 };
    return render_jobs(points, image, depth, N, W, H, baseline, n_frames, jobs, stages & ~(KBE_STAGE_ZBUF_A | KBE_STAGE_ZBUF_B), fill_rect, raster_w, raster_n,
                       (hipStream_t) stream);
}

int kbe_render_frame(const float* points, const float* image, const float* depth, int N, int W, int H, double focal,
                     double baseline, const float* shift3, void* scratch, uint8_t* frame_u8, float* render_f32,
                     float* existing_f32, float* zee_f32, float* zee_pre_f32, kbe_stream_t stream)
{
    return kbe_render_frame_stages(points, image, depth, N, W, H, focal, baseline, shift3, scratch, frame_u8, render_f32,
                                   existing_f32, zee_f32, zee_pre_f32, KBE_STAGE_PROJECT | KBE_STAGE_TILES | KBE_STAGE_FILL,
                                   nullptr, 0, 0, stream);
}

int kbe_render_frame_fused(const void* packed, int N, double cloud_focal, int W, int H, double focal, double baseline,
                           const float* shift3, void* scratch, uint8_t* frame_u8, float* render_f32, float* existing_f32,
                           float* zee_f32, float* zee_pre_f32, int stages, const int* fill_rect, int parity, kbe_stream_t stream)
{
    KBE_REQUIRE(packed && scratch && frame_u8 && N >= 0 && N <= KBE_FUSED_MAX_POINTS && frame_size_ok(W, H) && ((uintptr_t) scratch & 15) == 0 &&
                cloud_focal > 0.0 && parity >= -1 && parity <= 1, "kbe_render_frame_fused: bad arguments");
    const hipStream_t s = (hipStream_t) stream;
    FusedTarget t = fused_target(scratch, W, H, focal, baseline, shift3, parity, frame_u8, -1);
    t.render_f32 = render_f32; t.existing_f32 = existing_f32; t.zee_f32 = zee_f32; t.zee_pre_f32 = zee_pre_f32;
    if (parity < 0 && !(stages & KBE_STAGE_KEEP_HOLE_COUNT))
        if (int rc = zero_hole_count(t.sc, s, "kbe_render_frame_fused: hipMemsetAsync")) return rc;
    return render_fused(s, packed, N, cloud_focal, 1, &t, false, 0, nullptr, stages, fused_build_of_stages(stages), fill_rect_of(fill_rect, W, H), 0.0,
                        "kbe_render_frame_fused");
}

int kbe_render_frame_group_fused(const void* packed, int N, double cloud_focal, int W, int H, double baseline, int n_frames, const double* focals,
                                 const float* shifts, void* const* scratch, uint8_t* const* frames_u8, const int* parities, int stages,
                                 const int* fill_rect, kbe_stream_t stream)
{
    KBE_REQUIRE(packed && n_frames >= 1 && n_frames <= KBE_FRAME_JOBS && focals && shifts && scratch && frames_u8 && N >= 0 && N <= KBE_FUSED_MAX_POINTS &&
                frame_size_ok(W, H) && cloud_focal > 0.0, "kbe_render_frame_group_fused: bad arguments");
    if (int rc = check_sets(n_frames, scratch, frames_u8, nullptr, "kbe_render_frame_group_fused: bad scratch / frame pointer",
                            "kbe_render_frame_group_fused: the frames of a group need scratch sets of their own"))
        return rc;
    const hipStream_t s = (hipStream_t) stream;
    FusedTarget ft[KBE_FRAME_JOBS];
    for (int k = 0; k < n_frames; k++) {
        const int par = parities ? parities[k] : -1;
        KBE_REQUIRE(par >= -1 && par <= 1, "kbe_render_frame_group_fused: parity is -1, 0 or 1");
        ft[k] = fused_target(scratch[k], W, H, focals[k], baseline, shifts + 3 * (size_t) k, par, frames_u8[k], -1);
    }
    // (every argument has been checked: only now is anything enqueued)
    for (int k = 0; k < n_frames; k++)
        if (ft[k].parity < 0 && !(stages & KBE_STAGE_KEEP_HOLE_COUNT))
            if (int rc = zero_hole_count(ft[k].sc, s, "kbe_render_frame_group_fused: hipMemsetAsync")) return rc;
    return render_fused(s, packed, N, cloud_focal, n_frames, ft, false, 0, nullptr, stages, fused_build_of_stages(stages), fill_rect_of(fill_rect, W, H), 0.0,
                        "kbe_render_frame_group_fused");
}

int kbe_render_frame_group_ahead_ok(int N, int W, int H, int n_frames, int n_next)
{
    return (N >= 0 && W > 0 && H > 0 && n_frames >= 1 && n_frames <= KBE_FRAME_JOBS && n_next >= 1 && n_next <= KBE_FRAME_JOBS &&
            fused_can_place_ahead(N, W, H, n_frames, n_next)) ? 1 : 0;
}

int kbe_render_frame_group_ahead(const void* packed, int N, double cloud_focal, int W, int H, double baseline, int n_frames, const double* focals,
                                 const float* shifts, void* const* scratch, uint8_t* const* frames_u8, const int* turns, int placed, int n_next,
                                 const double* next_focals, const float* next_shifts, void* const* next_scratch, const int* next_turns, int stages,
                                 const int* fill_rect, double near_depth, kbe_stream_t stream)
{
    KBE_REQUIRE(packed && n_frames >= 1 && n_frames <= KBE_FRAME_JOBS && focals && shifts && scratch && frames_u8 && turns && N >= 0 && N <= KBE_FUSED_MAX_POINTS &&
                frame_size_ok(W, H) && cloud_focal > 0.0, "kbe_render_frame_group_ahead: bad arguments");
    KBE_REQUIRE(n_next >= 0 && n_next <= KBE_FRAME_JOBS && (n_next == 0 || (next_focals && next_shifts && next_scratch && next_turns)), "kbe_render_frame_group_ahead: bad next group");
    KBE_REQUIRE(near_depth >= 0.0 && near_depth < 1.0e30, "kbe_render_frame_group_ahead: near_depth is a depth (0: unknown)");
    KBE_REQUIRE(n_next == 0 || fused_can_place_ahead(N, W, H, n_frames, n_next), "kbe_render_frame_group_ahead: too many placements for the tile launch (kbe_render_frame_group_ahead_ok)");
    const char* const twice = "kbe_render_frame_group_ahead: the frames of a group need scratch sets of their own";
    if (int rc = check_sets(n_frames, scratch, frames_u8, turns, "kbe_render_frame_group_ahead: bad scratch / frame pointer / turn", twice)) return rc;
    if (int rc = check_sets(n_next, next_scratch, nullptr, next_turns, "kbe_render_frame_group_ahead: bad scratch / turn of the next group", twice)) return rc;
    for (int k = 0; k < n_next; k++)
        for (int j = 0; j < n_frames; j++)
            KBE_REQUIRE(next_scratch[k] != scratch[j] || next_turns[k] == turns[j] + 1, "kbe_render_frame_group_ahead: a set used by both groups takes consecutive turns");
    const hipStream_t s = (hipStream_t) stream;
    FusedTarget ft[KBE_FRAME_JOBS], nt[KBE_FRAME_JOBS];
    for (int k = 0; k < n_frames; k++) ft[k] = fused_target(scratch[k], W, H, focals[k], baseline, shifts + 3 * (size_t) k, turns[k] & 1, frames_u8[k], turns[k]);
    for (int k = 0; k < n_next; k++)
        nt[k] = fused_target(next_scratch[k], W, H, next_focals[k], baseline, next_shifts + 3 * (size_t) k, next_turns[k] & 1, nullptr, next_turns[k]);
    // (every argument has been checked: only now is anything enqueued)
    // A set's first turn -- in this group, without placements made ahead, or joining the sequence with the next group -- starts from zero
    for (int k = 0; k < n_frames; k++)
        if (turns[k] == 0 && !placed)
            if (int rc = start_set(ft[k].sc, s, "kbe_render_frame_group_ahead: hipMemsetAsync")) return rc;
    for (int k = 0; k < n_next; k++)
        if (next_turns[k] == 0)
            if (int rc = start_set(nt[k].sc, s, "kbe_render_frame_group_ahead: hipMemsetAsync")) return rc;
    return render_fused(s, packed, N, cloud_focal, n_frames, ft, placed != 0, n_next, nt, stages, fused_build_of_stages(stages), fill_rect_of(fill_rect, W, H),
                        near_depth, "kbe_render_frame_group_ahead");
}

int kbe_render_pointcloud_tiled(const float* points, const float* data, int N, int C, int W, int H, double focal,
                                double baseline, const float* shift3, void* scratch, float* render, float* existing,
                                kbe_stream_t stream)
{
    KBE_REQUIRE(scratch && render && existing && N >= 0 && N <= (1 << 30) && C > 0 && frame_size_ok(W, H) && ((uintptr_t) scratch & 15) == 0,
                "kbe_render_pointcloud_tiled: bad arguments");
    KBE_REQUIRE(N == 0 || (points && data), "kbe_render_pointcloud_tiled: cloud pointers are NULL");
    const hipStream_t s = (hipStream_t) stream;
    const Scratch sc = carve(scratch, W, H);
    const Camera cam = make_camera(W, H, focal, baseline, shift3);
    const int n_tiles = sc.tiles_x * sc.tiles_y;
    int rc = kbe_render_frame_stages(points, data, data, N, W, H, focal, baseline, shift3, scratch, (uint8_t*) sc.holes, nullptr, nullptr,
                                     nullptr, nullptr, KBE_STAGE_PROJECT, nullptr, 0, 0, stream);
    if (rc != KBE_OK) return rc;
    TileNcArgs a;
    a.points = points; a.data = data; a.N = N; a.C = C; a.cam = cam;
    if (N == 0) a.points = a.data = (const float*) sc.zkeys;            // never dereferenced for a record, but never NULL
    a.zkeys = sc.zkeys; a.tile_count = sc.tile_count; a.buckets = sc.buckets; a.tiles_x = sc.tiles_x; a.tiles_y = sc.tiles_y;
    a.render = render; a.existing = existing;
    hipLaunchKernelGGL(k_tiles_nc, dim3(n_tiles), dim3(TILE_THREADS), 0, s, a);
    if ((rc = launched("kbe_render_pointcloud_tiled/tiles"))) return rc;
    // leave the scratch clean (z-buffer, bucket counters)
    hipLaunchKernelGGL(k_scratch_init, dim3(1024), dim3(256), 0, s, sc.zkeys, (uint32_t*) nullptr, (size_t) W * H, sc.tile_count, n_tiles, sc.hole_count);
    return launched("kbe_render_pointcloud_tiled/reset");
}

int kbe_render_video(const float* points, const float* image, const float* depth, int N, int W, int H, double baseline,
                     int n_frames, const double* focals, const float* shifts, int crop_w, int crop_h, void* scratch,
                     uint8_t* stage, int batch, uint8_t* host_out, int raster_w, int raster_n, const void* packed,
                     double cloud_focal, int flags, kbe_stream_t stream, kbe_stream_t copy_stream, int lanes,
                     const kbe_stream_t* lane_streams, double near_depth)
{
    KBE_REQUIRE(n_frames >= 0 && focals && shifts && stage && host_out && frame_size_ok(W, H) && batch >= -64 && (!packed || cloud_focal > 0.0),
                "kbe_render_video: bad arguments");
    KBE_REQUIRE((crop_w == 0 && crop_h == 0) || (crop_w > 0 && crop_h > 0 && crop_w <= W && crop_h <= H), "kbe_render_video: bad crop");
    KBE_REQUIRE(lanes >= 1 && lanes <= KBE_MAX_LANES && (lanes == 1 || lane_streams), "kbe_render_video: bad lanes");
    KBE_REQUIRE(near_depth >= 0.0 && near_depth < 1.0e30, "kbe_render_video: near_depth is a depth (0: unknown)");
    KBE_REQUIRE(scratch && ((uintptr_t) scratch & 15) == 0 && N >= 0 && (packed || (N <= (1 << 30) && (N == 0 || (points && image && depth)))),
                "kbe_render_video: bad scratch or cloud");
    const hipStream_t cs = (hipStream_t) stream;
    const size_t sb = (scratch_set_bytes(W, H, N) + 255) & ~(size_t) 255;      // == kbe_video_scratch_stride: lane stride
    const bool crop = crop_w > 0;
    // KBE_VIDEO_FILL_GROUP(n), n <= KBE_FILL_JOBS (`scratch` then holds n * lanes sets): a lane renders n frames, each into a
    // scratch set of its own, and fills them in the same launches.  The table-driven fill is bound by its own chain of
    // dependent look-ups, not by the chip (272 us alone, 352 us with four of them overlapping), and more than four
    // streams do not overlap any better (the hardware queues): several frames per launch are the way to have more in flight.
    // KBE_VIDEO_GROUP(n), n <= KBE_FRAME_JOBS, for the fused route, whose scatter launches take up to KBE_FRAME_JOBS frames (fill
    // and crop launches then take them four at a time)
    const int wide_group = ((flags >> 5) & 15) + 1;
    const int group = batch <= 0 ? (wide_group > 1 ? wide_group : ((flags >> 1) & 3) + 1) : 1;
    KBE_REQUIRE(group <= (packed ? KBE_FRAME_JOBS : KBE_FILL_JOBS), "kbe_render_video: more frames per launch than the route's launches take");
    KBE_REQUIRE(!packed || N <= KBE_FUSED_MAX_POINTS, "kbe_render_video: the packed cloud's route takes up to 2^28 points (more: the plain cloud's route)");
    // Frames are independent, so consecutive frames go to `lanes` HIP streams, each with its own scratch and raw
    // frame: the fixed cost of a kernel boundary on this chip (launch ramp, tail, and the L2 write-back between
    // dependent kernels) is then paid while another frame's kernels run.
    hipStream_t ls[KBE_MAX_LANES];
    for (int l = 0; l < lanes; l++) ls[l] = l == 0 ? cs : (hipStream_t) lane_streams[l];
    const StageLayout layout = stage_layout(W, H, lanes, batch, KBE_FRAME_JOBS);
    // how the frames leave (kbe_handoff.h); the staged ring (batch > 0) alone uses the copy stream
    VideoHandoff handoff;
    if (int rc0 = handoff.open(HandoffIn{ stage, layout, host_out, batch, flags, lanes, ls, copy_stream ? (hipStream_t) copy_stream : cs })) return rc0;
    int rect[4] = { 0, 0, W - 1, H - 1 };
    if (crop) {
        // the pixels cv2.getRectSubPix reads (common.py:256), padded by one: see kbe_render_frame_stages
        const int x0 = (int) floor(W / 2.0 - (crop_w - 1) * 0.5) - 1, y0 = (int) floor(H / 2.0 - (crop_h - 1) * 0.5) - 1;
        rect[0] = x0 > 0 ? x0 : 0; rect[1] = y0 > 0 ? y0 : 0;
        rect[2] = x0 + crop_w + 2 < W - 1 ? x0 + crop_w + 2 : W - 1;
        rect[3] = y0 + crop_h + 2 < H - 1 ? y0 + crop_h + 2 : H - 1;
    }
    if (packed) {
        // every scratch set starts the call on hole counter 0: its counters (and list totals) are zeroed here, on `stream`, before
        // the lanes start -- by ONE small launch for all sets (a memset per set was eight launches in front of a video's first frame)
        const Scratch sc0 = carve(scratch, W, H);
        hipLaunchKernelGGL(k_zero_counters, dim3(16, group * lanes), dim3(256), 0, cs, sc0.hole_count, sb, group * lanes, sc0.tile_count,
                           2 * align16(4 * (size_t) sc0.tiles_x * sc0.tiles_y * CNT_STRIDE) / sizeof(int));
        if (int rc0 = launched("kbe_render_video/counters")) return rc0;
    }
    const VideoPlan plan = plan_video(VideoPlanIn{ n_frames, lanes, group, batch, handoff.dest, layout.fin, (flags & KBE_VIDEO_FAST_RAMP) != 0, (flags & KBE_VIDEO_EVEN_GROUPS) != 0,
                                                   packed != nullptr, !(flags & KBE_VIDEO_NO_AHEAD) },
                                      [&](int n, int n_next) { return fused_can_place_ahead(N, W, H, n, n_next); });

    // ---- how a planned launch is enqueued: its frames scattered into scratch sets of their own, filled together, cropped
    const int in_flight = plan.single ? lanes : lanes * group;          // frames in flight
    const int fill_flags = in_flight >= KBE_FILL_BY_COUNT_MIN_LANES ? (KBE_STAGE_FILL_BY_COUNT | ((flags & KBE_VIDEO_FILL_DIST) ? KBE_STAGE_FILL_DIST : 0)) : 0;
    const int build = (flags & KBE_VIDEO_FUSED_LEAN) ? 1 : ((flags & KBE_VIDEO_FUSED_ROOMY) ? 2 : 0);
    const FillRect fill_rect = fill_rect_of(rect, W, H);
    // frame f of the fused route on its scratch set, its parity that of its turn
    auto fused_target_of = [&](const PlanFrame& f, uint8_t* frame, int turn) {
        return fused_target((char*) scratch + (size_t) f.set * sb, W, H, focals[f.frame], baseline, shifts + 3 * (size_t) f.frame, f.turn & 1, frame, turn);
    };
    auto render = [&](const PlanLaunch& a) {
        const hipStream_t s = ls[a.lane];
        const PlanFrame* const fr = &plan.frames[a.first];
        uint8_t* outs[KBE_FRAME_JOBS];
        uint8_t* raws[KBE_FRAME_JOBS];          // where the frames are rendered: the lane's raw frames when cropped
        for (int j = 0; j < a.count; j++) {
            outs[j] = handoff.slot(fr[j]);
            raws[j] = crop ? stage + layout.raw(a.lane, j) : outs[j];
        }
        int rc = KBE_OK;
        if (!packed) {
            // bucket route: every launch (projection, tiles, fill) takes all the frames
            FrameJob jobs[KBE_FILL_JOBS];
            for (int j = 0; j < a.count; j++)
                jobs[j] = FrameJob{ focals[fr[j].frame], shifts + 3 * (size_t) fr[j].frame, (char*) scratch + (size_t) fr[j].set * sb, raws[j], nullptr, nullptr, nullptr, nullptr,
                                    fr[j].zbuf == PLAN_ZBUF_A ? KBE_STAGE_ZBUF_A : (fr[j].zbuf == PLAN_ZBUF_B ? KBE_STAGE_ZBUF_B : 0) };
            rc = render_jobs(points, image, depth, N, W, H, baseline, a.count, jobs, KBE_STAGE_PROJECT | KBE_STAGE_TILES | KBE_STAGE_FILL | fill_flags, crop ? rect : nullptr, raster_w, raster_n, s);
        } else if (plan.single) {
            // the fused scatter on the packed cloud, one frame on its own (turn -1: its placements are made in front of it); a lane's
            // frames alternate between its two hole counters
            const FusedTarget t = fused_target_of(fr[0], raws[0], -1);
            rc = render_fused(s, packed, N, cloud_focal, 1, &t, false, 0, nullptr, KBE_STAGE_TILES | KBE_STAGE_FILL | fill_flags, build, fill_rect, 0.0, "kbe_render_video");
        } else {
            // fused route: the binning launch and the tile launch take all the frames, the fill four at a time; the tile launch also
            // makes the placements of the lane's next launch when the plan says so
            FusedTarget ft[KBE_FRAME_JOBS], nt[KBE_FRAME_JOBS];
            for (int j = 0; j < a.count; j++) ft[j] = fused_target_of(fr[j], raws[j], fr[j].turn);
            const int n_next = a.next >= 0 ? plan.launches[a.next].count : 0;
            const PlanFrame* const next = n_next ? &plan.frames[plan.launches[a.next].first] : nullptr;
            for (int j = 0; j < n_next; j++) nt[j] = fused_target_of(next[j], nullptr, next[j].turn);
            rc = render_fused(s, packed, N, cloud_focal, a.count, ft, a.placed, n_next, nt, KBE_STAGE_TILES | KBE_STAGE_FILL | fill_flags, build, fill_rect, near_depth,
                              "kbe_render_video");
        }
        for (int j0 = 0; j0 < a.count && rc == KBE_OK && crop; j0 += KBE_FILL_JOBS)
            rc = crop_resize_group(a.count - j0 < KBE_FILL_JOBS ? a.count - j0 : KBE_FILL_JOBS, raws + j0, W, H, crop_w, crop_h, outs + j0, s);
        return rc;
    };

    // ---- the plan, in order
    int rc = handoff.start(plan);
    for (int u = 0; u < (int) plan.units.size() && rc == KBE_OK; u++) {
        const PlanUnit& un = plan.units[u];
        handoff.before(u, un);
        for (int a = un.launch0; a < un.launch1 && rc == KBE_OK; a++) rc = render(plan.launches[a]);
        if (rc == KBE_OK) rc = handoff.after(u, un, plan);
    }
    return handoff.finish(rc, plan);
}

}  // extern "C"
