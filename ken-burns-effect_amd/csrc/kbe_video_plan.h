// The launch plan of kbe_render_video (kbe_frame.hip; its frames leave through kbe_handoff.hip): which lane renders which frames in
// which launch, into which scratch set and which destination slot, and how the frames leave -- decided on indices alone, before
// anything is enqueued -- and the layout of `stage`, which those slots index.  Plain C++ (no HIP): tests/video_plan_check.cpp checks
// its invariants on the host.
#pragma once
#include <stddef.h>
#include <vector>

namespace kbe {

enum class VideoDest {
    HBM,            // host_out is device memory: every frame's last kernel stores straight into host_out[i]
    PER_FRAME,      // batch == 0, pinned host memory: one frame per unit, k_deliver behind it
    GROUPS,         // batch < 0, pinned host memory: transfer groups of up to G = -batch consecutive frames, one lane each
    RING,           // batch > 0: round 1's staged ring, two halves of `batch` frames
};
enum { PLAN_ZBUF_ALONE = 0, PLAN_ZBUF_A = 1, PLAN_ZBUF_B = 2 };      // the bucket route's z-buffers (KBE_STAGE_ZBUF_*; 0: stand-alone)

// stage = [raw_per_lane * lanes raw frames][lanes * fin finished frames][ring half 0: batch frames][ring half 1: batch frames]
// [turn counter of the hand-off: 256 bytes, 256-byte aligned].  The raw frames are those of a cropped video in front of the crop (a
// launch takes up to raw_per_lane = KBE_FRAME_JOBS frames); PlanFrame::slot indexes the finished frames or the ring.
struct StageLayout {
    size_t fb;              // bytes of a frame
    int fin;                // finished-frame buffers per lane: two, or a whole transfer group's
    size_t raw_per_lane, finished, ring, ctl, total;    // the regions' byte offsets (raw frames: 0), and kbe_video_stage_bytes
    size_t raw(int lane, int j) const { return (raw_per_lane * lane + j) * fb; }        // frame j of the lane's launch
};
inline StageLayout stage_layout(int W, int H, int lanes, int batch, int raw_per_lane)
{
    const size_t fb = (size_t) W * H * 3, fin = batch < -2 ? -batch : 2;
    const size_t finished = (size_t) raw_per_lane * lanes * fb, ring = finished + fin * lanes * fb;
    const size_t ctl = (ring + 2 * (size_t) (batch > 0 ? batch : 0) * fb + 255) & ~(size_t) 255;
    return StageLayout{ fb, (int) fin, (size_t) raw_per_lane, finished, ring, ctl, ctl + 256 };
}

struct VideoPlanIn {
    int n_frames, lanes, group, batch;  // group: frames per launch (KBE_VIDEO_GROUP / _FILL_GROUP); batch: kbe_render_video's
    VideoDest dest;
    int fin;                // finished-frame buffers per lane (PER_FRAME, GROUPS)
    bool fast_ramp, even_groups;        // KBE_VIDEO_FAST_RAMP, KBE_VIDEO_EVEN_GROUPS
    bool fused;             // the packed cloud's route (else the bucket route)
    bool ahead;             // fused route: a launch may make the placements of its lane's next launch (no KBE_VIDEO_NO_AHEAD)
};
struct PlanFrame {
    int frame;              // index into the video
    int set;                // scratch set (single: the lane's; else group * lane + position in the launch)
    int turn;               // the set's uses before this one: the fused route's turn (parity turn & 1)
    int zbuf;               // PLAN_ZBUF_*: bucket route
    int slot;               // HBM: host_out[slot]; PER_FRAME, GROUPS: finished frame `slot`; RING: frame `slot` of the ring
};
struct PlanLaunch {
    int lane, first, count; // its frames: frames[first .. first + count)
    bool placed;            // its placements were made by the lane's previous launch
    int next;               // the launch whose placements this one makes ahead (the lane's next), or -1
};
struct PlanUnit {           // a transfer group, a ring half, a single delivered frame or an HBM chunk
    int lane;               // GROUPS, PER_FRAME: the lane that renders and sends it (else -1)
    int first, count;       // its frames of the video: first .. first + count - 1
    int launch0, launch1;   // its launches: launches[launch0 .. launch1)
};
struct VideoPlan {
    bool single;            // one frame per launch in the one-frame form (fused: turn -1, parity turn & 1; bucket: set = lane)
    std::vector<PlanUnit> units;
    std::vector<PlanLaunch> launches;
    std::vector<PlanFrame> frames;
};

// The transfer groups of the hand-off by groups: sizes 1, 2, 4, ... (fast ramp: 1, 3, 7, ...; even groups: all G) up to G = -batch,
// then G.  The link is idle until the first group has been rendered, and a transfer costs ~25 us whatever its size: a video of 20
// frames in groups of 2 ran at 41 GB/s, in groups of 16 it would wait for 16 frames before the first byte moves.  Small groups
// first start the link after one frame; the groups double while it is busy.  starts[g] .. starts[g + 1]: the frames of group g.
inline std::vector<int> transfer_group_starts(int n_frames, int G, bool fast_ramp, bool even_groups)
{
    std::vector<int> starts;
    for (int i0 = 0, size = even_groups ? G : 1; i0 < n_frames; ) {
        starts.push_back(i0);
        i0 += size < n_frames - i0 ? size : n_frames - i0;
        const int grown = fast_ramp ? size * 2 + 1 : size * 2;
        size = grown < G ? grown : G;
    }
    starts.push_back(n_frames);
    return starts;
}

// can_place_ahead(n, n_next): may a launch of n frames make the placements of n_next more (kbe_fused_plan.h: fused_can_place_ahead)
template <class CanPlaceAhead>
VideoPlan plan_video(const VideoPlanIn& in, CanPlaceAhead can_place_ahead)
{
    VideoPlan p;
    p.single = in.dest == VideoDest::PER_FRAME || in.dest == VideoDest::RING || (in.group == 1 && !in.fused);
    const int per = p.single ? 1 : in.group;                    // frames per launch
    std::vector<int> uses((size_t) in.lanes * in.group, 0);     // per scratch set
    auto unit = [&](int lane, int first, int count) { p.units.push_back(PlanUnit{ lane, first, count, (int) p.launches.size(), (int) p.launches.size() }); };
    // a launch of frames i0, i0 + 1, ... (n of them) on lane l, into slots s0, s0 + 1, ...
    auto launch = [&](int l, int i0, int n, int s0) {
        p.launches.push_back(PlanLaunch{ l, (int) p.frames.size(), n, false, -1 });
        for (int j = 0; j < n; j++) {
            const int set = p.single ? l : in.group * l + j;
            p.frames.push_back(PlanFrame{ i0 + j, set, uses[set]++, PLAN_ZBUF_ALONE, s0 + j });
        }
        p.units.back().launch1++;
    };
    const int n = in.n_frames;
    switch (in.dest) {
    case VideoDest::HBM:
        // a chunk of per * lanes CONSECUTIVE frames at a time, lane l taking frames base + l * per .. base + l * per + per - 1 of it
        // (consecutive cameras share candidate lists, kbe_fused_plan.h: share_plan; until round 5 lane l took frames l, l + lanes, ...:
        // cameras `lanes` steps apart in every launch: 40.4 k frames/s at 75 frames, 40.8 k consecutive).  The last, partial chunk fills the
        // lanes one after the other, `per` frames each.  (ADVICE r5 proposed to deal it evenly, ceil(remaining / lanes) frames per lane, so that every lane
        // has work: measured in round 6 -- tools/batches/gpu_r06_tail.sh, frames/s left in HBM, lane by lane / evenly: 6 frames 26.5 /
        // 26.4 k, 8: 29.5 / 29.5, 12: 33.5 / 33.4, 20: 35.9 / 33.9, 24: 37.6 / 35.5, 30: 38.2 / 37.7, 40: 39.8 / 39.6 -- never faster,
        // 5 % slower where it turns one four-frame launch into four one-frame launches: a launch's ramp and tail cost more than the
        // idle lanes.)
        for (int base = 0; base < n; base += per * in.lanes) {
            unit(-1, base, (n - base < per * in.lanes ? n - base : per * in.lanes));
            for (int l = 0, i0 = base; l < in.lanes && i0 < n; l++, i0 += per) launch(l, i0, n - i0 < per ? n - i0 : per, i0);
        }
        break;
    case VideoDest::PER_FRAME:          // a lane alternates between its finished-frame slots
        for (int i = 0; i < n; i++) { unit(i % in.lanes, i, 1); launch(i % in.lanes, i, 1, i % (in.fin * in.lanes)); }
        break;
    case VideoDest::GROUPS: {           // group g goes to lane g % lanes, which renders it into its own fin slots
        const std::vector<int> starts = transfer_group_starts(n, -in.batch, in.fast_ramp, in.even_groups);
        for (size_t g = 0; g + 1 < starts.size(); g++) {
            const int l = (int) g % in.lanes, i0 = starts[g], nb = starts[g + 1] - i0;
            unit(l, i0, nb);
            for (int k = 0; k < nb; k += per) launch(l, i0 + k, nb - k < per ? nb - k : per, l * in.fin + k);
        }
        break;
    }
    case VideoDest::RING:               // the halves alternate; frame i on lane i % lanes
        for (int i0 = 0, h = 0; i0 < n; i0 += in.batch, h ^= 1) {
            const int nb = n - i0 < in.batch ? n - i0 : in.batch;
            unit(-1, i0, nb);
            for (int k = 0; k < nb; k++) launch((i0 + k) % in.lanes, i0 + k, 1, h * in.batch + k);
        }
        break;
    }
    // the bucket route: a set's frames alternate between its two z-buffers (A, B, A, ...), each clearing the other's in its tile
    // launch; a set's LAST frame, if it falls on A, takes the stand-alone form (A cleared by its fill launch), so that every call
    // leaves A empty -- B is always cleared before it is used.  (The last frame by COUNT: with groups of G frames per lane
    // `i + lanes >= n_frames` named frames in the middle of a lane's share, which then ran stand-alone and left B dirty for the
    // lane's next frame.)
    for (PlanFrame& f : p.frames) f.zbuf = (f.turn & 1) ? PLAN_ZBUF_B : (f.turn + 1 == uses[f.set] ? PLAN_ZBUF_ALONE : PLAN_ZBUF_A);
    // the fused route: a launch's tile launch also makes the placements of the lane's next launch (its set j then takes its next
    // turn) -- not for a next launch that is LARGER: that is the ramp of the transfer groups at the start of a delivered video, where
    // the first frames should leave as early as they can (a one-frame launch that also places four frames holds the first transfer
    // back: --steps 20 14.1 k -> 13.4 k frames/s with it)
    std::vector<int> last(in.lanes, -1);                        // the lane's previous launch
    for (int a = 0; a < (int) p.launches.size() && in.fused && in.ahead && !p.single; a++) {
        PlanLaunch& cur = p.launches[a];
        const int b = last[cur.lane];
        last[cur.lane] = a;
        if (b >= 0 && cur.count <= p.launches[b].count && can_place_ahead(p.launches[b].count, cur.count)) { p.launches[b].next = a; cur.placed = true; }
    }
    return p;
}

}  // namespace kbe
