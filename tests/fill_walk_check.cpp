// Host checker of ken-burns-effect_amd/csrc/kbe_fill_walk.h (tests/test_fill_tables_cpu.py builds and runs it): the header's own
// functions -- the ones the kernels of kbe_holes.hip are compiled from -- against brute force.
//   advance           m fp32 additions taken on the integer mantissa (Axis, advance_exact) against the additions one at a time
//   strips MASK.u8    on a 1024 x 1024 validity mask (one byte per pixel): the strip tables and the pass test, k_dead and the jump
//                     lengths against brute-force walks
//   tile              strip_bounds on one tile with two valid pixels: exact
//   key               the contest key: round trip, order by length, then direction
//   plan              stdin: lines "W H stages tiles_x tiles_y" -> fill_plan's fields, one line each
//   g++ -O2 -std=c++17 -ffp-contract=off -I ken-burns-effect_amd/csrc -I include tests/fill_walk_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kbe_fill_walk.h"

using namespace kbe;

namespace {

constexpr int TW = 32, TH = 16;             // kbe_tiles.h: KBE_TILE_W, KBE_TILE_H
struct Dirs { float x[16], y[16]; };
Dirs fill_dirs()                            // common.py:859-867, as kbe_fill.h's make_fill_dirs
{
    const float dx[16] = { -1, 0, 1, 1, -1, 1, 2, 2, -2, -1, 1, 2, 3, 3, 3, 3 }, dy[16] = { 1, 1, 1, 0, 2, 2, 1, -1, 3, 3, 3, 3, 2, 1, -1, -2 };
    Dirs d;
    for (int i = 0; i < 16; i++) { volatile float n = sqrtf(dx[i] * dx[i] + dy[i] * dy[i]); d.x[i] = dx[i] / n; d.y[i] = dy[i] / n; }
    return d;
}
uint32_t g_seed = 12345;
uint32_t rnd() { return (g_seed = g_seed * 1664525u + 1013904223u) >> 8; }

// starts 0..11000 -- the longest side the tables take (fill_tables_fit), every start of the binade that begins at 8192 and of the
// tables' last 16 pixels among them -- (+ offs[d], if given), twelve legs of up to 250 steps of us[d] in either sense: the walk as the kernel takes it against
// the additions one at a time
struct AdvanceCounts { long walks, advances, catch_ups, bad; };
bool sweep_advance(const float* us, const float* offs, int n_us, AdvanceCounts& n)
{
    long& walks = n.walks; long& advances = n.advances; long& catch_ups = n.catch_ups; long& bad = n.bad;
    for (int d = 0; d < n_us; d++) {
        for (int sub = 0; sub < 2; sub++) for (int start = 0; start <= 11000; start += (start < 1100 || (start >= 8176 && start < 8208) || start >= 10984 ? 1 : 7)) {
            const float u = us[d], first = (float) start + (offs ? offs[d] : 0.0f);
            Axis A = axis_enter(first, u, sub);
            volatile float seq = first;
            int total = 0;
            walks++;
            for (int leg = 0; leg < 12; leg++) {
                const int m = (int) rnd() % ((leg & 1) ? 250 : 9) + 1;
                for (int k = 0; k < m; k++) seq = sub ? seq - u : seq + u;
                total += m;
                int r = m;
                axis_jump(A, r);
                for (int guard = 0; r > 0; guard++) {
                    axis_catch_up(A, r, u, sub, 20000.0f);
                    catch_ups++;
                    if (guard > 1000) { printf("stuck\n"); return false; }
                }
                advances++;
                if (seq < -1.0f || seq > 20000.0f) break;           // the kernel stops caring here
                const float got = axis_value(A), want = seq;
                const float ex = advance_exact(first, u, total, sub, INFINITY), ex_lim = advance_exact(first, u, total, sub, 20000.0f);
                if (f32_bits(got) != f32_bits(want) || f32_bits(ex) != f32_bits(want) || f32_bits(ex_lim) != f32_bits(want) || axis_pixel(A) != (int) roundf(want)) {
                    if (bad++ < 5) printf("MISMATCH u=%.9g sub=%d start=%.9g after %d steps: axis %.9g (pixel %d), advance_exact %.9g / %.9g, one at a time %.9g\n",
                                          (double) u, sub, (double) first, total, (double) got, axis_pixel(A), (double) ex, (double) ex_lim, (double) want);
                }
            }
        }
    }
    return true;
}

int check_advance()
{
    // the 16 fill directions, both axes
    const Dirs D = fill_dirs();
    float us[32];
    for (int d = 0; d < 16; d++) { us[2 * d] = D.x[d]; us[2 * d + 1] = D.y[d]; }
    AdvanceCounts n = {}, t = {};
    if (!sweep_advance(us, nullptr, 32, n)) return 1;
    printf("walks %ld, advances %ld (catch-ups %ld), mismatches %ld\n", n.walks, n.advances, n.catch_ups, n.bad);
    // Steps that are ties in some binade of the image (u an odd multiple of 2^-k: half-way between two neighbours of the grid of
    // [2^(24-k), 2^(25-k)), where round-to-even looks at the value), from starts that are odd on that grid.  The fill itself never
    // gets there -- from a pixel's integer coordinate every tie rounds to an even value -- but the functions promise any start.
    float ties[40], offs[40];
    int n_ties = 0;
    for (int k = 11; k <= 20; k++) for (int v = 0; v < 4; v++) { offs[n_ties] = ldexpf(1.0f, 1 - k); ties[n_ties++] = (v & 1 ? 0.3125f : 0.6875f) + (v & 2 ? 3.0f : 1.0f) * ldexpf(1.0f, -k); }
    if (!sweep_advance(ties, offs, n_ties, t)) return 1;
    printf("ties: walks %ld, advances %ld (catch-ups %ld), mismatches %ld\n", t.walks, t.advances, t.catch_ups, t.bad);
    return n.bad != 0 || t.bad != 0;
}

constexpr int W = 1024, H = 1024, TX = W / TW, TY = H / TH, CW = W / 8, CH = H / 8;
struct Box { int x, y, z, w; };
uint8_t m[H][W];

// Chebyshev distance to the nearest set cell, capped: by brute-force dilation
std::vector<uint8_t> distances(const std::vector<uint8_t>& set, int w, int h, int cap)
{
    std::vector<uint8_t> dist((size_t) w * h, (uint8_t) cap), cur = set, next((size_t) w * h);
    for (size_t i = 0; i < cur.size(); i++) if (cur[i]) dist[i] = 0;
    for (int k = 1; k < cap; k++) {
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
            uint8_t v = 0;
            for (int dy = -1; dy <= 1 && !v; dy++) for (int dx = -1; dx <= 1 && !v; dx++) {
                const int xx = x + dx, yy = y + dy;
                if (xx >= 0 && xx < w && yy >= 0 && yy < h) v = cur[(size_t) yy * w + xx];
            }
            next[(size_t) y * w + x] = v;
            if (v && !cur[(size_t) y * w + x]) dist[(size_t) y * w + x] = (uint8_t) k;
        }
        cur.swap(next);
    }
    return dist;
}

// one end of a ray from (x, y), step by step (common.py:876-889): valid[k - 1] = the pixel k steps on is valid, up to the first valid
// pixel or, `to_border`, the image border
void walk(int x, int y, float ux, float uy, bool plus, bool to_border, std::vector<uint8_t>& valid)
{
    valid.clear();
    volatile float fx = (float) x, fy = (float) y;
    for (;;) {
        fx = plus ? fx + ux : fx - ux; fy = plus ? fy + uy : fy - uy;
        const int ix = (int) roundf(fx), iy = (int) roundf(fy);
        if (ix < 0 || ix >= W || iy < 0 || iy >= H) return;
        valid.push_back(m[iy][ix]);
        if (m[iy][ix] && !to_border) return;
    }
}

int check_strips(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f || fread(m, 1, sizeof(m), f) != sizeof(m)) { printf("cannot read %s\n", path); return 2; }
    fclose(f);
    const Dirs D = fill_dirs();
    // what the tile launch leaves: the box of every tile's valid pixels, the validity bitmask
    std::vector<Box> bbox((size_t) TX * TY, Box{ W, H, -1, -1 });
    std::vector<uint32_t> bits((size_t) H * (W / 32), 0u);
    std::vector<uint8_t> px_set((size_t) W * H), blk_set((size_t) CW * CH, 0);
    int bx0 = W, bx1 = -1, by0 = H, by1 = -1;
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        px_set[(size_t) y * W + x] = m[y][x];
        if (!m[y][x]) continue;
        Box& q = bbox[(size_t) (y / TH) * TX + x / TW];
        q.x = imin(q.x, x); q.y = imin(q.y, y); q.z = imax(q.z, x); q.w = imax(q.w, y);
        bx0 = imin(bx0, x); bx1 = imax(bx1, x); by0 = imin(by0, y); by1 = imax(by1, y);
        bits[(size_t) y * (W / 32) + (x >> 5)] |= 1u << (x & 31);
        blk_set[(size_t) (y >> 3) * CW + (x >> 3)] = 1;
    }
    const std::vector<uint8_t> dist = distances(px_set, W, H, 15), dist_blocks = distances(blk_set, CW, CH, 15);      // k_hole_dist's two tables
    const int bins = strip_bins(W, H);
    std::vector<float> lo((size_t) 16 * bins), hi((size_t) 16 * bins);
    int off[16];
    for (int d = 0; d < 16; d++) {
        off[d] = strip_offset(D.x[d], D.y[d], W, H);
        for (int b = 0; b < bins; b++) strip_bounds<TW, TH>(b, bbox.data(), bits.data(), TX, TY, W, H, D.x[d], D.y[d], lo[(size_t) d * bins + b], hi[(size_t) d * bins + b]);
    }
    long holes = 0, pairs = 0, complete = 0, survive = 0, false_kills = 0, bad_bins = 0;
    long dead_ends = 0, dead_steps = 0, dead_bad = 0, jump_walks = 0, jump_skipped = 0, jump_bad = 0, jump_stuck = 0;
    std::vector<uint8_t> va, vb;
    for (int y = by0; y <= by1; y++) for (int x = bx0; x <= bx1; x++) {
        if (m[y][x]) continue;
        holes++;
        const bool sampled = x % 4 == 0 && y % 4 == 0;              // k_dead and the jumps: every sixteenth hole
        for (int d = 0; d < 16; d++) {
            const float ux = D.x[d], uy = D.y[d];
            pairs++;
            walk(x, y, ux, uy, false, sampled, va); walk(x, y, ux, uy, true, sampled, vb);
            const auto first_hit = [](const std::vector<uint8_t>& v) { for (size_t k = 0; k < v.size(); k++) if (v[k]) return (long) k + 1; return 0l; };
            const long ka = first_hit(va), kb = first_hit(vb);
            const bool comp = ka && kb;                             // both ends reach a valid pixel before leaving the image
            complete += comp;
            const float c = strip_across(ux, uy, x, y), t = strip_along(ux, uy, x, y);
            const int b = strip_line(c) + off[d];
            if (b < 0 || b >= bins) { bad_bins++; continue; }
            const float l = lo[(size_t) d * bins + b], h = hi[(size_t) d * bins + b];
            const bool surv = !strip_skip(l, h, t);
            survive += surv;
            if (comp && !surv) { if (false_kills++ < 6) printf("FALSE KILL x=%d y=%d d=%d c=%.3f t=%.3f b=%d lo=%.3f hi=%.3f\n", x, y, d, c, t, b, l, h); }
            if (!sampled) continue;
            for (int end = 0; end < 2; end++) {
                const std::vector<uint8_t>& v = end ? vb : va;
                // an end declared dead never later meets a valid pixel
                const int k_dead = strip_k_dead(end ? h - t : t - l);
                if (k_dead <= (int) v.size()) {
                    dead_ends++;
                    for (size_t k = (size_t) imax(k_dead, 1); k <= v.size(); k++) { dead_steps++; if (v[k - 1]) { if (dead_bad++ < 6) printf("DEAD END MEETS x=%d y=%d d=%d end=%d k_dead=%d k=%zu\n", x, y, d, end, k_dead, k); break; } }
                }
                // no position skipped by a jump is valid: the walk of k_fill_tables' step(), then with the pixel table alone (its creep())
                for (int mode = 0; mode < 2; mode++) {
                    const float inv_umax = jump_inv_umax(ux, uy);
                    volatile float fx = (float) x, fy = (float) y;
                    const int c_here = dist_blocks[(size_t) (y >> 3) * CW + (x >> 3)];
                    int jump = (c_here >= 2 && mode == 0) ? first_jump_from_blocks(c_here) : first_jump_from_pixels(dist[(size_t) y * W + x]);
                    long k = 0;
                    jump_walks++;
                    for (;;) {
                        if (jump < 1) { jump_stuck++; break; }
                        bool out = false;
                        for (int j = 1; j <= jump && !out; j++) {
                            fx = end ? fx + ux : fx - ux; fy = end ? fy + uy : fy - uy;
                            k++;
                            if (k > (long) v.size()) { out = true; break; }
                            if (j < jump) { jump_skipped++; if (v[k - 1]) { if (jump_bad++ < 6) printf("JUMP SKIPS VALID x=%d y=%d d=%d end=%d mode=%d k=%ld\n", x, y, d, end, mode, k); } }
                        }
                        if (out || v[k - 1]) break;                 // left the image / landed on a valid pixel
                        const int ix = (int) roundf(fx), iy = (int) roundf(fy);
                        const int cb = dist_blocks[(size_t) (iy >> 3) * CW + (ix >> 3)], dn = dist[(size_t) iy * W + ix];
                        if (mode == 0) jump = cb >= KBE_FILL_FINE_BELOW ? jump_from_blocks(cb, inv_umax) : imax(cb >= 2 ? jump_from_blocks(cb, inv_umax) : 1, jump_from_pixels(dn, inv_umax));
                        else jump = imax(1, jump_from_pixels(dn, inv_umax));
                    }
                }
            }
        }
    }
    printf("holes in box %ld, pairs %ld, complete %ld (%.2f/hole), survive strip test %ld (%.2f/hole), false kills %ld, bins out of range %ld\n",
           holes, pairs, complete, (double) complete / holes, survive, (double) survive / holes, false_kills, bad_bins);
    printf("dead ends %ld, steps walked beyond %ld, valid pixels met %ld\n", dead_ends, dead_steps, dead_bad);
    printf("jump walks %ld, positions skipped %ld, valid pixels skipped %ld, jumps of no step %ld\n", jump_walks, jump_skipped, jump_bad, jump_stuck);
    return 0;
}

// One tile with two valid pixels in opposite corners: its box is the whole tile, so the boxes alone bound every strip that crosses
// the tile; looked at row by row -- it is the tile that reaches farthest at either end -- the bound is exact: a strip without a
// valid pixel is empty (+inf, -inf: every hole on it skips the direction), a strip with one is bounded by that pixel
int check_one_tile()
{
    const int w = 512, h = 256, tx = w / TW, ty = h / TH, x0 = 10 * TW, y0 = 10 * TH;
    const int px[2] = { x0, x0 + TW - 1 }, py[2] = { y0, y0 + TH - 1 };
    std::vector<Box> bbox((size_t) tx * ty, Box{ w, h, -1, -1 });
    std::vector<uint32_t> bits((size_t) h * (w / 32), 0u);
    bbox[(size_t) 10 * tx + 10] = Box{ px[0], py[0], px[1], py[1] };
    for (int i = 0; i < 2; i++) bits[(size_t) py[i] * (w / 32) + (px[i] >> 5)] |= 1u << (px[i] & 31);
    const Dirs D = fill_dirs();
    long empty = 0, empty_bounded = 0, holding = 0, holding_wrong = 0;
    for (int d = 0; d < 16; d++) for (int b = 0; b < strip_bins(w, h); b++) {
        float lo, hi;
        strip_bounds<TW, TH>(b, bbox.data(), bits.data(), tx, ty, w, h, D.x[d], D.y[d], lo, hi);
        const float c0 = (float) (b - strip_offset(D.x[d], D.y[d], w, h)) - STRIP_MARGIN, c1 = c0 + 1.0f + 2.0f * STRIP_MARGIN;
        bool none = true, clear = true;         // no pixel in or near the strip / every pixel clearly in or clearly out
        float tmin = INFINITY, tmax = -INFINITY;
        for (int i = 0; i < 2; i++) {
            const float c = strip_across(D.x[d], D.y[d], px[i], py[i]), t = strip_along(D.x[d], D.y[d], px[i], py[i]);
            if (c > c0 - 0.05f && c < c1 + 0.05f) none = false;
            if (c > c0 + 0.05f && c < c1 - 0.05f) { tmin = fminf(tmin, t); tmax = fmaxf(tmax, t); }
            else if (c > c0 - 0.05f && c < c1 + 0.05f) clear = false;
        }
        if (none) { empty++; if (lo != INFINITY || hi != -INFINITY) { if (empty_bounded++ < 6) printf("EMPTY STRIP BOUNDED d=%d b=%d lo=%.3f hi=%.3f\n", d, b, lo, hi); } }
        else if (clear) { holding++; if (fabsf(lo - tmin) > 0.01f || fabsf(hi - tmax) > 0.01f) { if (holding_wrong++ < 6) printf("STRIP NOT EXACT d=%d b=%d lo=%.3f hi=%.3f pixels %.3f .. %.3f\n", d, b, lo, hi, tmin, tmax); } }
    }
    printf("one tile: empty strips %ld (bounded all the same %ld), strips with a pixel %ld (not bounded by it %ld)\n", empty, empty_bounded, holding, holding_wrong);
    return empty_bounded || holding_wrong;
}

int check_key()
{
    struct Entry { float length; int d, ka, kb; unsigned long long key; };
    std::vector<Entry> es;
    long bad_trip = 0, bad_order = 0, compared = 0;
    for (int i = 0; i < 20000; i++) {
        const int ex = (int) (rnd() % 64), ey = (int) (rnd() % 64);     // spans of few pixels: many equal lengths
        Entry e = { sqrtf((float) (ex * ex + ey * ey)) * ((i & 3) ? 1.0f : 97.0f), (int) (rnd() % 16), (int) (rnd() % (FILL_MAX_STEPS + 1)), (int) (rnd() % (FILL_MAX_STEPS + 1)), 0ull };
        if (i % 1000 == 0) { e.ka = FILL_MAX_STEPS; e.kb = FILL_MAX_STEPS; e.d = 15; }
        e.key = fill_key_pack(e.length, e.d, e.ka, e.kb);
        const FillKey k = fill_key_unpack(e.key);
        if (k.d != e.d || k.ka != e.ka || k.kb != e.kb || f32_bits(e.length) != (uint32_t) (e.key >> 32) || e.key >= FILL_NO_ENTRY) bad_trip++;
        es.push_back(e);
    }
    for (size_t i = 0; i + 1 < es.size(); i++) for (size_t j = i + 1; j < es.size() && j < i + 40; j++) {
        const Entry& a = es[i]; const Entry& b = es[j];
        compared++;
        if (a.length != b.length) { if ((a.length < b.length) != (a.key < b.key)) bad_order++; }
        else if (a.d != b.d) { if ((a.d < b.d) != (a.key < b.key)) bad_order++; }
    }
    printf("key: entries %zu, round trips bad %ld, pairs compared %ld, order bad %ld\n", es.size(), bad_trip, compared, bad_order);
    return bad_trip || bad_order;
}

int print_plans()
{
    int w, h, stages, tx, ty;
    while (scanf("%d %d %d %d %d", &w, &h, &stages, &tx, &ty) == 5) {
        const FillPlan P = fill_plan<TW, TH>(w, h, stages, tx, ty);
        const int arg = fill_tables_arg(P.tables, P.min_holes);
        // which of a frame with min_holes - 1, min_holes, min_holes + 1 holes k_fill_holes still has to fill
        printf("%d %d %d %d %d %d %d %u %u %d %d%d%d\n", P.fill_mode, (int) P.tables, P.min_holes, P.use_strips, P.dist_gx, P.dist_gy, P.image_rows, P.tables_blocks, P.fill_blocks,
               arg, (int) fill_tables_left(arg, P.min_holes - 1), (int) fill_tables_left(arg, P.min_holes), (int) fill_tables_left(arg, P.min_holes + 1));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "advance")) return check_advance();
    if (!strcmp(what, "strips") && argc > 2) return check_strips(argv[2]);
    if (!strcmp(what, "key")) return check_key();
    if (!strcmp(what, "tile")) return check_one_tile();
    if (!strcmp(what, "plan")) return print_plans();
    fprintf(stderr, "usage: fill_walk_check advance | strips MASK.u8 | tile | key | plan\n");
    return 2;
}
