// Host-side checker of kbe_render_video's launch plan and stage layout (ken-burns-effect_amd/csrc/kbe_video_plan.h), run by
// tests/test_video_plan.py.
//   video_plan_check                  every invariant over a sweep of videos; prints "<plans checked> <failures>"
//   video_plan_check DEST N LANES GROUP BATCH FLAGS
//                                     prints one plan: a "unit LANE FIRST COUNT" line per unit, then its launches as
//                                     "launch LANE PLACED NEXT FRAME:SET:TURN:ZBUF:SLOT ..."; DEST 0..3 = HBM, PER_FRAME, GROUPS, RING;
//                                     FLAGS: 1 fast ramp, 2 even groups, 4 fused route, 8 placements ahead
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kbe_video_plan.h"

using namespace kbe;

static bool can_place_ahead(int n, int n_next) { return n + n_next <= 14; }     // a stand-in for fused_can_place_ahead: some pairs may not

static const int RAW_PER_LANE = 12;                 // the most frames a launch takes (kbe_tiles.h: KBE_FRAME_JOBS; the sweep's groups go up to it)
static StageLayout layout_of(int lanes, int batch) { return stage_layout(5 + lanes, 3, lanes, batch, RAW_PER_LANE); }      // (frames of an odd size)

static VideoPlanIn make_in(int dest, int n, int lanes, int group, int batch, int flags)
{
    const int fin = layout_of(lanes, batch).fin;
    return VideoPlanIn{ n, lanes, group, batch, (VideoDest) dest, fin, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0 };
}

static long failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, "dest %d n %d lanes %d group %d batch %d flags %d: ", \
    (int) in.dest, in.n_frames, in.lanes, in.group, in.batch, flags); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } return; } } while (0)

static void check(const VideoPlanIn& in, int flags)
{
    const VideoPlan p = plan_video(in, can_place_ahead);
    const int per = p.single ? 1 : in.group;
    CHECK(p.single == (in.dest == VideoDest::PER_FRAME || in.dest == VideoDest::RING || (in.group == 1 && !in.fused)), "single form");
    // every frame exactly once, units consecutive, launches inside their unit
    std::vector<int> seen(in.n_frames, 0);
    int next_first = 0, next_launch = 0;
    std::vector<int> starts;                        // the transfer groups' ramp, as kbe.h documents it
    for (int i0 = 0, size = in.even_groups ? -in.batch : 1; in.dest == VideoDest::GROUPS && i0 < in.n_frames; ) {
        starts.push_back(i0);
        i0 += size;
        size = in.fast_ramp ? 2 * size + 1 : 2 * size;
        if (size > -in.batch) size = -in.batch;
    }
    for (int u = 0; u < (int) p.units.size(); u++) {
        const PlanUnit& un = p.units[u];
        CHECK(un.first == next_first && un.count >= 1 && un.launch0 == next_launch && un.launch1 > un.launch0, "unit %d not consecutive", u);
        next_first += un.count; next_launch = un.launch1;
        if (in.dest == VideoDest::GROUPS) {
            CHECK(u < (int) starts.size() && un.first == starts[u], "transfer group %d starts at %d", u, un.first);
            CHECK(un.lane == u % in.lanes, "transfer group %d on lane %d", u, un.lane);
        }
        if (in.dest == VideoDest::PER_FRAME) CHECK(un.count == 1 && un.lane == un.first % in.lanes, "per-frame unit %d", u);
        if (in.dest == VideoDest::RING) CHECK(un.first == u * in.batch && un.count <= in.batch, "ring half %d", u);
        if (in.dest == VideoDest::HBM) CHECK(un.first % (per * in.lanes) == 0 && un.count <= per * in.lanes, "HBM chunk %d", u);
        int expect = un.first;
        for (int a = un.launch0; a < un.launch1; a++) {
            const PlanLaunch& la = p.launches[a];
            CHECK(la.count >= 1 && la.count <= per, "launch %d takes %d frames", a, la.count);
            if (in.dest == VideoDest::GROUPS || in.dest == VideoDest::PER_FRAME) CHECK(la.lane == un.lane, "launch %d off its unit's lane", a);
            if (in.dest == VideoDest::HBM) CHECK(la.lane == a - un.launch0 && la.count == (un.first + un.count - expect < per ? un.first + un.count - expect : per),
                                                 "HBM launch %d: lane l takes base + l * group + m", a);
            if (in.dest == VideoDest::RING) CHECK(la.lane == expect % in.lanes, "ring launch %d on lane %d", a, la.lane);
            for (int j = 0; j < la.count; j++) {
                const PlanFrame& f = p.frames[la.first + j];
                CHECK(f.frame == expect, "launch %d: frame %d where %d was due", a, f.frame, expect);
                expect++;
                CHECK(f.frame >= 0 && f.frame < in.n_frames && !seen[f.frame]++, "frame %d twice", f.frame);
                CHECK(f.set == (p.single ? la.lane : in.group * la.lane + j), "frame %d in set %d", f.frame, f.set);
                const int k = f.frame - un.first;
                const int slot = in.dest == VideoDest::HBM ? f.frame : in.dest == VideoDest::PER_FRAME ? f.frame % (in.fin * in.lanes)
                               : in.dest == VideoDest::GROUPS ? la.lane * in.fin + k : (u & 1) * in.batch + k;
                CHECK(f.slot == slot, "frame %d in slot %d", f.frame, f.slot);
                if (in.dest == VideoDest::GROUPS) CHECK(k < in.fin, "transfer group %d overruns its lane's slots", u);
            }
        }
        CHECK(expect == un.first + un.count, "unit %d's launches do not cover it", u);
    }
    // the stage: its regions in order, without gaps or overlap, the turn counter 256-byte aligned behind the last frame; every slot's
    // frame, and every raw frame of a launch, wholly inside its region
    const StageLayout L = layout_of(in.lanes, in.batch);
    const size_t ring_end = L.ring + 2 * (size_t) (in.batch > 0 ? in.batch : 0) * L.fb;
    CHECK(L.fin == in.fin && L.raw(in.lanes - 1, RAW_PER_LANE - 1) + L.fb == L.finished && L.finished + (size_t) L.fin * in.lanes * L.fb == L.ring, "stage regions");
    CHECK(L.ctl >= ring_end && L.ctl < ring_end + 256 && L.ctl % 256 == 0 && L.total == L.ctl + 256, "turn counter at %zu", L.ctl);
    for (const PlanLaunch& la : p.launches)
        for (int j = 0; j < la.count; j++) {
            const PlanFrame& f = p.frames[la.first + j];
            CHECK(L.raw(la.lane, j) + L.fb <= L.finished, "frame %d: raw frame outside its region", f.frame);
            const size_t lo = in.dest == VideoDest::RING ? L.ring : L.finished, hi = in.dest == VideoDest::RING ? ring_end : L.ring;
            if (in.dest != VideoDest::HBM) CHECK(f.slot >= 0 && lo + ((size_t) f.slot + 1) * L.fb <= hi, "frame %d: slot %d outside its region of the stage", f.frame, f.slot);
        }
    CHECK(next_first == in.n_frames, "the units cover %d of %d frames", next_first, in.n_frames);
    CHECK(next_launch == (int) p.launches.size(), "launches outside every unit");
    // turns count a set's uses; the bucket route's z-buffers: every frame splats into a clear one, and A is clear at the end
    std::vector<int> uses(in.lanes * in.group, 0);
    std::vector<char> a_dirty(uses.size(), 0), b_dirty(uses.size(), 0);
    for (const PlanFrame& f : p.frames) {
        CHECK(f.turn == uses[f.set]++, "frame %d: turn %d", f.frame, f.turn);
        if (f.zbuf == PLAN_ZBUF_B) { CHECK(!b_dirty[f.set], "frame %d splats into a dirty B", f.frame); b_dirty[f.set] = 1; a_dirty[f.set] = 0; }
        else { CHECK(!a_dirty[f.set], "frame %d splats into a dirty A", f.frame); a_dirty[f.set] = f.zbuf == PLAN_ZBUF_A; if (f.zbuf == PLAN_ZBUF_A) b_dirty[f.set] = 0; }
        CHECK(f.zbuf == PLAN_ZBUF_A || f.zbuf == PLAN_ZBUF_B || f.zbuf == PLAN_ZBUF_ALONE, "frame %d: z-buffer %d", f.frame, f.zbuf);
    }
    for (size_t s = 0; s < uses.size(); s++) CHECK(!a_dirty[s], "set %d ends the call with z-buffer A dirty", (int) s);
    // placements ahead: only into the same lane's next launch, never a larger one, within the bound; the sets take consecutive turns
    std::vector<int> placed_by(p.launches.size(), -1);
    for (int a = 0; a < (int) p.launches.size(); a++) {
        const PlanLaunch& la = p.launches[a];
        if (la.next < 0) continue;
        CHECK(in.fused && in.ahead && !p.single, "launch %d places ahead on a route that does not", a);
        CHECK(la.next > a && la.next < (int) p.launches.size(), "launch %d places ahead into launch %d", a, la.next);
        const PlanLaunch& nx = p.launches[la.next];
        CHECK(nx.lane == la.lane && nx.count <= la.count && can_place_ahead(la.count, nx.count), "launch %d places ahead into launch %d", a, la.next);
        for (int b = a + 1; b < la.next; b++) CHECK(p.launches[b].lane != la.lane, "launch %d places ahead past the lane's next launch", a);
        for (int j = 0; j < nx.count; j++)
            CHECK(p.frames[nx.first + j].set == p.frames[la.first + j].set && p.frames[nx.first + j].turn == p.frames[la.first + j].turn + 1,
                  "launch %d: the sets placed ahead do not take consecutive turns", a);
        placed_by[la.next] = a;
    }
    for (int a = 0; a < (int) p.launches.size(); a++) CHECK(p.launches[a].placed == (placed_by[a] >= 0), "launch %d: placed %d", a, (int) p.launches[a].placed);
    // with the placements allowed, a lane's next launch that may take them does
    if (in.fused && in.ahead && !p.single) {
        std::vector<int> last(in.lanes, -1);
        for (int a = 0; a < (int) p.launches.size(); a++) {
            const int b = last[p.launches[a].lane];
            last[p.launches[a].lane] = a;
            if (b >= 0 && p.launches[a].count <= p.launches[b].count && can_place_ahead(p.launches[b].count, p.launches[a].count))
                CHECK(p.launches[b].next == a, "launch %d does not place ahead into launch %d", b, a);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc == 7) {
        const int flags = atoi(argv[6]);
        const VideoPlanIn in = make_in(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), flags);
        const VideoPlan p = plan_video(in, can_place_ahead);
        for (const PlanUnit& un : p.units) {
            printf("unit %d %d %d\n", un.lane, un.first, un.count);
            for (int a = un.launch0; a < un.launch1; a++) {
                const PlanLaunch& la = p.launches[a];
                printf("launch %d %d %d", la.lane, (int) la.placed, la.next);
                for (int j = 0; j < la.count; j++) {
                    const PlanFrame& f = p.frames[la.first + j];
                    printf(" %d:%d:%d:%d:%d", f.frame, f.set, f.turn, f.zbuf, f.slot);
                }
                printf("\n");
            }
        }
        return 0;
    }
    long plans = 0;
    const int G[] = { 1, 2, 3, 4, 5, 8, 12, 16, 31, 64 }, B[] = { 1, 2, 5, 16, 64 };
    for (int n = 0; n <= 140; n++)
        for (int lanes = 1; lanes <= 8; lanes++)
            for (int group = 1; group <= 12; group++)
                for (int flags = 0; flags < 16; flags++) {
                    if ((flags & 8) && !(flags & 4)) continue;          // placements ahead: the fused route's
                    check(make_in(0, n, lanes, group, 0, flags), flags); plans++;
                    check(make_in(1, n, lanes, group, 0, flags), flags); plans++;
                    for (int g : G) { check(make_in(2, n, lanes, group, -g, flags), flags); plans++; }
                    if (group == 1) for (int b : B) { check(make_in(3, n, lanes, group, b, flags), flags); plans++; }
                }
    printf("%ld %ld\n", plans, failures);
    return failures ? 1 : 0;
}
