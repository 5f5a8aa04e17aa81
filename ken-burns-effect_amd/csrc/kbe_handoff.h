// kbe_handoff.h -- how the finished frames of a kbe_render_video call reach the caller (kbe_handoff.hip): one object per call.
// kbe_render_video (kbe_frame.hip) opens it, has every frame's last kernel store into slot(), and walks its plan's units:
//     before(u, unit); the unit's launches; after(u, unit, plan);          and at the end, whatever happened, finish(rc, plan).
// Everything behind that -- the kernels that copy and take turns, the SDMA engine and the process-wide pool of its signals, the
// events between the lanes, the clean-up after an error -- is the module's own.
#pragma once
#include "kbe_host.h"
#include "kbe_video_plan.h"

namespace kbe {

struct HandoffIn {
    uint8_t* stage;             // kbe_render_video's, laid out as `layout`
    StageLayout layout;
    uint8_t* host_out;
    int batch, flags;           // kbe_render_video's
    int lanes;
    const hipStream_t* ls;      // the lanes' streams; ls[0] is the call's `stream`
    hipStream_t dc;             // the staged ring's copy stream (`stream` if the caller gave none)
};

struct VideoHandoff : HandoffIn {
    VideoHandoff();
    ~VideoHandoff();
    // where do the frames go (a host_out the runtime does not know is taken for device memory)?  Zeroes the turn counter, where there
    // is one, on `stream`.  KBE_OK, or the error of a host_out that is host memory the device cannot address, or of a misaligned stage
    int open(const HandoffIn& in);
    uint8_t* slot(const PlanFrame& f) const { return slots + (size_t) f.slot * layout.fb; }     // where the frame's last kernel stores
    // the other streams start once everything enqueued on `stream` so far (the cloud) is done; the ring's events
    int start(const VideoPlan& plan);
    void before(int u, const PlanUnit& un);                         // the lanes wait until the unit's slots are free
    int after(int u, const PlanUnit& un, const VideoPlan& plan);    // send the unit after its launches
    // the lanes wait for their last groups to have left; after an error no copy outlives the call; whoever synchronises `stream`
    // afterwards also sees every frame delivered and every other stream idle.  Returns the call's status
    int finish(int rc, const VideoPlan& plan);

    VideoDest dest;
    // ---- the rest is kbe_handoff.hip's
    uint8_t* host_dev;          // host_out as the device sees it, when it is pinned host memory
    uint8_t* slots;             // slot 0: host_out, the finished frames or the ring
    int turn_polls;
    bool sdma_asked, ok;        // ok: every event could be created
    volatile int64_t* lane_fin[KBE_MAX_LANES];          // the completion signal of the group the lane's slots hold
    // events (created and destroyed per call): `start`, per slot / ring half `rendered` and `copied`, per stream `idle`
    static constexpr int MAX_EV = 4 + 4 * KBE_MAX_LANES;
    hipEvent_t pool[MAX_EV], rendered[2][KBE_MAX_LANES], copied[2];
    int n_ev;
    struct Hidden;              // what needs the module's own types: the call's use of the SDMA engine, the turn counter, the dev builds' trace
    Hidden* const hid;          // (lives in `hidden`: no allocation)
    alignas(16) unsigned char hidden[256];
    hipEvent_t make();
    void join();
    int send_group(int u, const PlanUnit& un, const VideoPlan& plan);
};

}  // namespace kbe
