// kbe_handoff.hip -- how the finished frames of a kbe_render_video call (kbe_frame.hip) reach the caller: the kernels that copy and
// take turns (k_deliver, k_turn), the hand-off by an SDMA engine (k_signal_release, k_signal_wait, the process-wide pool of its
// signals, kbe_video_handoff_status), and VideoHandoff (kbe_handoff.h), one call's use of all of it.  The rules that keep it safe:
//   - a copy on the engine is released by the kernel behind its group's launches; SdmaPair::released says that this kernel is known
//     to be in the stream, and sdma_abort releases from the host every copy of a failed call for which it is not;
//   - after an error sdma_abort runs before the lanes are joined; always, sdma_close records on `stream` behind the join when the
//     call's pairs are idle again, and only then are the call's events destroyed;
//   - a pair is idle again once that event has passed (sdma_open looks), or at once when the engine never took its copy.
#include <chrono>
#include <mutex>
#include <new>
#include <thread>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include "kbe_handoff.h"

using namespace kbe;

#if defined(KBE_VIDEO_TRACE)
#include <time.h>
#define KBE_HOST_TRACE(...) __VA_ARGS__
static double trace_now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
#else
#define KBE_HOST_TRACE(...)
#endif
#if defined(KBE_VIDEO_GPU_TRACE)
#define KBE_GPU_TRACE(...) __VA_ARGS__
#else
#define KBE_GPU_TRACE(...)
#endif

namespace {

// ---------------------------------------------------------------------------------------
// frame hand-off (common.py:255 `.cpu()`): finished uint8 frames go from the lane's device buffers into pinned host
// memory IN THE LANE'S OWN STREAM -- no copy stream, no event (cross-stream events cost ~25 us per frame on this
// stack: a dedicated copy stream measured 89-107 us per frame) -- either by the runtime's transfer engine, one
// hipMemcpyAsync per group of frames (default), or by k_deliver below, one frame at a time.
// Left alone, the lanes' copies share the PCIe link, finish together, and the lanes then render together: a convoy
// that leaves the link idle a quarter of the time (measured: 80 us per 1024^2 frame, 39 GB/s).  So the copies take
// TURNS: copy i waits (one lane polling, s_sleep in between) until copy i - 1 has finished and then has the link
// to itself; the lanes fall into a staggered pipeline -- with two lanes, one renders its next group while the other's
// group leaves -- and the link is busy back to back (59 us per frame = 53 GB/s of the ~57 the link gives a single
// large transfer; tools/d2h_probe*.hip, gpurun_out sweeps in DESIGN.md).  The turn is ADVISORY -- a performance
// ordering only: the wait is bounded (~4 ms) and a copy that gives up simply copies, so no mapping of streams onto
// hardware queues can deadlock it.
// k_deliver: a copy kernel with plain 16-byte stores into device-visible host memory.  64 unthrottled workgroups
// reach 55 GB/s alone, but PCIe-bound stores parked in the write queues stall every other kernel's stores; 16
// workgroups with 2 KB in flight per wave are the best compromise found (66 us per frame next to 3 rendering lanes).
// ---------------------------------------------------------------------------------------
constexpr int DELIVER_BLOCKS = 16, DELIVER_THREADS = 256, DELIVER_KB_PER_WAVE = 2;
constexpr int DELIVER_MAX_POLLS = 4096;     // x ~1 us
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct DeliverCtl { uint32_t serving; uint32_t pad[31]; uint32_t done[32]; };
static_assert(sizeof(DeliverCtl) <= 256, "kbe_video_stage_bytes reserves 256 bytes");      // serving: copies finished so far; done: per-copy workgroup count

// the turn of a runtime transfer.  pass == 0: the group draws a ticket NOW, when its frames are ready -- first ready, first
// served: with turns in the order of the groups a lane whose group is ready waited for lanes still rendering earlier groups
// (dolly frames differ 5 x in cost along a video: passes of 109 and 145 ms alternated) -- and waits (bounded) until the
// transfers in front of it have finished; pass == 1 hands the turn on.  pad[0]: tickets drawn so far.
__global__ void __launch_bounds__(64) k_turn(DeliverCtl* ctl, int pass, int max_polls)
{
    if (threadIdx.x != 0) return;
    if (pass) { atomicAdd(&ctl->serving, 1u); return; }
    const uint32_t ticket = atomicAdd(&ctl->pad[0], 1u);
    for (int polls = 0; polls < max_polls; polls++) {
        if (__hip_atomic_load(&ctl->serving, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= ticket) break;
        __builtin_amdgcn_s_sleep(32);
    }
}

// ---------------------------------------------------------------------------------------
// The hand-off by an SDMA ENGINE (KBE_VIDEO_SDMA; round 5).  hipMemcpyAsync device-to-host is a blit KERNEL on this runtime:
// it takes wave slots next to the rendering and sits in the lane's stream, so the lane's next group cannot start before its
// last one has left.  HSA drives the DMA engines directly (hsa_amd_memory_async_copy_on_engine), and a copy can be ordered
// against HIP streams from the GPU side alone (tools/sdma_probe.hip): the host enqueues the copy of a group at once with a
// DEPENDENCY signal the engine polls, a one-lane kernel behind the group's last launch stores 0 into that signal's value, and
// whoever needs the copy done -- the lane before it renders into the same slots again, `stream` at the end of the call -- runs
// a one-lane kernel that polls the copy's COMPLETION signal.  The engine takes the copies in the order they were enqueued:
// the lanes need no turns.  The signals live in a process-wide pool (the one piece of state the library keeps: they must
// outlive the call, which returns before the copies run) and are reused once the call that used them has run to its end.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_signal_release(volatile int64_t* value)
{
    if (threadIdx.x != 0) return;
    __threadfence_system();
    __hip_atomic_store((int64_t*) value, (int64_t) 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// bounded (SDMA_WAIT_SECONDS of the device's wall clock -- the rate is asked of the runtime, sdma_wait_ticks -- where a video's groups take
// milliseconds): an engine that never reports is a dead or a stalled device, and a kernel that polls for ever would hide that.  Giving up
// is an ERROR the caller must see -- the frames of that group are not in its memory -- but not one to kill the process for (a trap raises
// an HSA queue exception and the runtime aborts: ADVICE r5): the kernel stores 1 into the pool's host-visible error word and returns.
// kbe_video_handoff_status() reports it (sticky) and waits on the host for the copies still under way; calls after it keep off the engine.
__global__ void __launch_bounds__(64) k_signal_wait(volatile int64_t* value, unsigned long long max_ticks, int* gave_up)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    do {
        if (__hip_atomic_load((int64_t*) value, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) <= 0) return;
        __builtin_amdgcn_s_sleep(16);
    } while (__builtin_amdgcn_s_memrealtime() - t0 < max_ticks);
    __hip_atomic_store(gave_up, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // (1 = not yet reported: kbe_video_handoff_status)
}
#ifndef KBE_SDMA_WAIT_SECONDS
#define KBE_SDMA_WAIT_SECONDS 4.0
#endif

struct SdmaPair {                       // the signals of one copy and where their values live
    hsa_signal_t dep, fin; volatile int64_t* dep_value; volatile int64_t* fin_value;
    bool released;                      // this use: the kernel that releases `dep` is known to be in a stream (else: the error path releases it from the host)
};
struct SdmaGeneration { hipEvent_t done; std::vector<SdmaPair> pairs; };
struct SdmaRoute { hsa_agent_t gpu, cpu; uint32_t engines; };          // the engines that copy from `gpu` to `cpu`'s memory (the preferred ones, or all)
struct SdmaPool {
    std::mutex mu;
    int state = 0;                              // 0 = not tried, 1 = HSA is up, -1 = it is not (or an engine stopped answering: no more copies through it)
    std::vector<SdmaPair> idle;
    std::vector<SdmaGeneration> running;
    std::vector<SdmaRoute> routes;
    int* gave_up = nullptr;                     // pinned host word, device-visible: a k_signal_wait that gave up stores 1 (sticky)
    unsigned long long wait_ticks = 0;          // KBE_SDMA_WAIT_SECONDS of the device's wall clock
};
static SdmaPool& sdma_pool() { static SdmaPool* p = new SdmaPool; return *p; }         // (never destroyed: the signals must not die before the runtime)
// A signal whose value device code may store to and poll: HSA asks for one that only GPUs consume (no host interrupt behind it -- nothing
// on the host ever waits for these) and hands out the value's address (hsa_amd_signal_value_pointer)
static bool sdma_signal(hsa_signal_t& sg, volatile int64_t*& value)
{
    if (hsa_amd_signal_create(1, 0, nullptr, HSA_AMD_SIGNAL_AMD_GPU_ONLY, &sg) != HSA_STATUS_SUCCESS) return false;
    volatile hsa_signal_value_t* p = nullptr;
    if (hsa_amd_signal_value_pointer(sg, &p) != HSA_STATUS_SUCCESS || !p) { (void) hsa_signal_destroy(sg); return false; }
    static_assert(sizeof(hsa_signal_value_t) == sizeof(int64_t), "a signal's value is 64 bits");
    value = (volatile int64_t*) p;
    return true;
}
struct SdmaCall {                               // one kbe_render_video call's use of the engine
    bool ok = false;
    hsa_agent_t gpu = {}, cpu = {};
    hsa_amd_sdma_engine_id_t engine = HSA_AMD_SDMA_ENGINE_0;
    std::vector<SdmaPair> used;
};
// which agents own the two buffers, and an engine that copies from the one to the other; false: no SDMA hand-off (the caller
// falls back to hipMemcpyAsync)
static bool sdma_open(SdmaCall& c, const void* device_buffer, const void* host_buffer)
{
    SdmaPool& pool = sdma_pool();
    std::lock_guard<std::mutex> lock(pool.mu);
    if (pool.state == 0) {
        pool.state = hsa_init() == HSA_STATUS_SUCCESS ? 1 : -1;       // (reference-counted: HIP's own runtime holds it up already)
        if (pool.state > 0) {
            // the word a polling kernel that gives up writes, and how many ticks of the wall clock it polls for (s_memrealtime counts at the
            // rate the runtime reports: 100 MHz on gfx950)
            int dev = 0, khz = 0;
            void* w = nullptr;
            if (hipHostMalloc(&w, 64, hipHostMallocMapped) != hipSuccess) { (void) hipGetLastError(); pool.state = -1; }
            else {
                pool.gave_up = (int*) w; *pool.gave_up = 0;
                if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) { (void) hipGetLastError(); khz = 100000; }
                pool.wait_ticks = (unsigned long long) (KBE_SDMA_WAIT_SECONDS * 1000.0 * (double) khz);
            }
        }
    }
    if (pool.state < 0) return false;
    if (__atomic_load_n(pool.gave_up, __ATOMIC_ACQUIRE) != 0) return false;      // an engine stopped answering: the runtime's transfers from here on
    hsa_amd_pointer_info_t dinfo = {}, hinfo = {};
    dinfo.size = hinfo.size = sizeof(hsa_amd_pointer_info_t);
    if (hsa_amd_pointer_info(device_buffer, &dinfo, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || dinfo.type == HSA_EXT_POINTER_TYPE_UNKNOWN) return false;
    if (hsa_amd_pointer_info(host_buffer, &hinfo, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || hinfo.type == HSA_EXT_POINTER_TYPE_UNKNOWN) return false;
    hsa_device_type_t dt, ht;
    if (hsa_agent_get_info(dinfo.agentOwner, HSA_AGENT_INFO_DEVICE, &dt) != HSA_STATUS_SUCCESS || dt != HSA_DEVICE_TYPE_GPU) return false;
    if (hsa_agent_get_info(hinfo.agentOwner, HSA_AGENT_INFO_DEVICE, &ht) != HSA_STATUS_SUCCESS || ht != HSA_DEVICE_TYPE_CPU) return false;
    // which engines copy from this GPU to this CPU agent is a property of the machine: asked once per pair of agents (the two queries cost
    // the host ~10 us of every call, between the launches of a video's first and second group)
    uint32_t pick = 0;
    for (const SdmaRoute& r : pool.routes)
        if (r.gpu.handle == dinfo.agentOwner.handle && r.cpu.handle == hinfo.agentOwner.handle) pick = r.engines;
    if (!pick) {
        uint32_t avail = 0, preferred = 0;
        if (hsa_amd_memory_copy_engine_status(hinfo.agentOwner, dinfo.agentOwner, &avail) != HSA_STATUS_SUCCESS || !avail) return false;
        if (hsa_amd_memory_get_preferred_copy_engine(hinfo.agentOwner, dinfo.agentOwner, &preferred) != HSA_STATUS_SUCCESS) preferred = 0;
        pick = (preferred & avail) ? (preferred & avail) : avail;
        pool.routes.push_back(SdmaRoute{ dinfo.agentOwner, hinfo.agentOwner, pick });
    }
    // its lowest engine.  (An engine takes ~9.4 us from the end of one copy to the start of the next even when that one has long been
    // released -- the device-side timeline of a 20-frame video, tools/sdma_timeline.py: five such gaps in 1.35 ms.  With the groups
    // alternating between TWO engines the copies overlap and the last one ends 60 us earlier on the device --
    // and the video is delivered SLOWER: 13.9 instead of 14.6 k frames/s for 20 frames, 16.15 instead of 16.6 k for 75: the host sees
    // the end ~170 us after the device instead of ~30.  One engine it is.)
    c.engine = (hsa_amd_sdma_engine_id_t) (pick & (~pick + 1u));
    c.gpu = dinfo.agentOwner; c.cpu = hinfo.agentOwner;
    // the signals of calls that have run to their end are idle again
    for (size_t g = 0; g < pool.running.size(); ) {
        if (hipEventQuery(pool.running[g].done) == hipSuccess) {
            (void) hipEventDestroy(pool.running[g].done);
            pool.idle.insert(pool.idle.end(), pool.running[g].pairs.begin(), pool.running[g].pairs.end());
            pool.running[g] = std::move(pool.running.back());
            pool.running.pop_back();
        } else {
            (void) hipGetLastError();       // hipErrorNotReady is not an error here
            g++;
        }
    }
    return c.ok = true;
}
static bool sdma_pair(SdmaCall& c, SdmaPair& p)
{
    SdmaPool& pool = sdma_pool();
    std::lock_guard<std::mutex> lock(pool.mu);
    if (!pool.idle.empty()) { p = pool.idle.back(); pool.idle.pop_back(); }
    else {
        if (!sdma_signal(p.dep, p.dep_value)) return false;
        if (!sdma_signal(p.fin, p.fin_value)) { (void) hsa_signal_destroy(p.dep); return false; }
    }
    hsa_signal_store_relaxed(p.dep, 1);
    hsa_signal_store_relaxed(p.fin, 1);
    p.released = false;
    c.used.push_back(p);
    return true;
}
// The call ends in an ERROR with copies on the engine (a launch failed behind them, KBE_VIDEO_INJECT_FAULT): none of them may outlive
// the call -- the caller, told of the error, may free its buffer the moment we return -- and none may keep waiting for a release
// that never comes (the engine's queue would be wedged for the process).  Every copy whose release kernel is not known to be in a
// stream is released from the host (it moves whatever its slots hold: the frames of a failed call are not valid anyway); the lanes
// run dry; the host polls every completion signal; a pair whose copy has completed is idle again, one whose copy has not after
// seconds is never reused.
static void sdma_abort(SdmaCall& c, const hipStream_t* lanes_streams, int lanes)
{
    if (c.used.empty()) return;
    for (SdmaPair& p : c.used) if (!p.released) hsa_signal_store_screlease(p.dep, 0);
    for (int l = 0; l < lanes; l++) { (void) hipStreamSynchronize(lanes_streams[l]); (void) hipGetLastError(); }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<SdmaPair> done;
    for (SdmaPair& p : c.used) {
        bool fin = false;
        while (!(fin = hsa_signal_load_scacquire(p.fin) <= 0) && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < KBE_SDMA_WAIT_SECONDS)
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        if (fin) done.push_back(p);
    }
    SdmaPool& pool = sdma_pool();
    std::lock_guard<std::mutex> lock(pool.mu);
    if (done.size() != c.used.size()) { __atomic_store_n(pool.gave_up, 1, __ATOMIC_RELEASE); pool.state = -1; }      // an engine that does not answer
    pool.idle.insert(pool.idle.end(), done.begin(), done.end());
    c.used.clear();
    c.ok = false;
}
// the call is enqueued: its signals are idle again once `stream` has run past this point
static void sdma_close(SdmaCall& c, hipStream_t stream)
{
    if (c.used.empty()) return;
    SdmaPool& pool = sdma_pool();
    std::lock_guard<std::mutex> lock(pool.mu);
    SdmaGeneration g;
    g.pairs.swap(c.used);
    if (hipEventCreateWithFlags(&g.done, hipEventDisableTiming) == hipSuccess && hipEventRecord(g.done, stream) == hipSuccess) pool.running.push_back(std::move(g));
    // (else: the pairs are dropped -- a leak of a few signals, never a reuse that is too early)
}

__global__ void __launch_bounds__(DELIVER_THREADS) k_deliver(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t bytes,
                                                             DeliverCtl* ctl, uint32_t ticket)
{
    if (ctl) {
        if (threadIdx.x == 0) {
            for (int polls = 0; polls < DELIVER_MAX_POLLS; polls++) {
                if (__hip_atomic_load(&ctl->serving, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= ticket) break;
                __builtin_amdgcn_s_sleep(32);
            }
        }
        __syncthreads();
    }
    const size_t gtid = (size_t) blockIdx.x * blockDim.x + threadIdx.x, gsz = (size_t) gridDim.x * blockDim.x;
    if ((((uintptr_t) src | (uintptr_t) dst) & 15) == 0) {          // uniform; the normal case (W*H*3 a multiple of 16)
        const size_t n16 = bytes >> 4;
        const u32x4* s16 = (const u32x4*) src;
        u32x4* d16 = (u32x4*) dst;
        // at most DELIVER_KB_PER_WAVE KB of stores in flight per wave: the link is fed (its bandwidth-delay product is
        // ~100 KB) without parking megabytes of PCIe-bound writes in the L2 / fabric write queues, where every
        // other kernel's stores wait behind them (measured: k_tiles 19 -> 89 us next to an unthrottled 64-workgroup copy)
        for (size_t i0 = gtid; i0 < n16; i0 += gsz * DELIVER_KB_PER_WAVE) {
#pragma unroll
            for (int k = 0; k < DELIVER_KB_PER_WAVE; k++) {
                const size_t i = i0 + (size_t) k * gsz;
                if (i < n16) d16[i] = __builtin_nontemporal_load(s16 + i);      // the frame is read once: no L2 allocation
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        for (size_t i = (n16 << 4) + gtid; i < bytes; i += gsz) dst[i] = src[i];
    } else {
        for (size_t i = gtid; i < bytes; i += gsz) dst[i] = src[i];
    }
    if (ctl) {
        // the last workgroup to get here passes the turn on (its own stores need not have landed: the next copy only
        // competes for the link, it does not read them)
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t* cnt = &ctl->done[ticket & 31];
            if (atomicAdd(cnt, 1u) == gridDim.x - 1) {
                __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                atomicMax(&ctl->serving, ticket + 1);
            }
        }
    }
}

// Dev builds only, the transfer groups of the hand-off: -DKBE_VIDEO_TRACE, where does the host spend the call (tools/handoff_trace.py);
// -DKBE_VIDEO_GPU_TRACE, when, on the device, a group's frames are ready, its gate opens, its transfer ends (tools/handoff_gpu_trace.py).
// Without either every hook is empty.
struct VideoTrace {
    KBE_HOST_TRACE(double t_call = trace_now(), t_g = 0, t_r = 0, t_t = 0, t_c = 0;)
    KBE_GPU_TRACE(hipEvent_t ev_start = nullptr; std::vector<hipEvent_t> ev_begin, ev_ready, ev_gate, ev_copied;)
    void start(int n_groups, hipStream_t cs)
    {
        KBE_GPU_TRACE(ev_begin.resize(n_groups); ev_ready.resize(n_groups); ev_gate.resize(n_groups); ev_copied.resize(n_groups);
                      (void) hipEventCreate(&ev_start); (void) hipEventRecord(ev_start, cs);
                      for (int g = 0; g < n_groups; g++) { (void) hipEventCreate(&ev_begin[g]); (void) hipEventCreate(&ev_ready[g]); (void) hipEventCreate(&ev_gate[g]); (void) hipEventCreate(&ev_copied[g]); })
    }
    void begin(int g, hipStream_t s) { KBE_GPU_TRACE((void) hipEventRecord(ev_begin[g], s);) KBE_HOST_TRACE(t_g = trace_now();) }
    void ready(int g, hipStream_t s) { KBE_HOST_TRACE(t_r = trace_now();) KBE_GPU_TRACE((void) hipEventRecord(ev_ready[g], s);) }
    void gate(int g, hipStream_t s) { KBE_GPU_TRACE((void) hipEventRecord(ev_gate[g], s);) KBE_HOST_TRACE(t_t = trace_now();) }
    void copied(int g, hipStream_t s) { KBE_GPU_TRACE((void) hipEventRecord(ev_copied[g], s);) KBE_HOST_TRACE(t_c = trace_now();) }
    void sent(int g, const PlanUnit& un)
    {
        KBE_HOST_TRACE(fprintf(stderr, "group %3d lane %d frames %3d..%3d: t=%8.1f us  render-enqueue %7.1f  turn %6.1f  hipMemcpyAsync %7.1f  turn %6.1f\n", g, un.lane, un.first,
                               un.first + un.count - 1, (t_g - t_call) * 1e6, (t_r - t_g) * 1e6, (t_t - t_r) * 1e6, (t_c - t_t) * 1e6, (trace_now() - t_c) * 1e6);)
    }
    void finish(const VideoPlan& plan, const hipStream_t* ls, int lanes, size_t fb, int rc)
    {
        KBE_GPU_TRACE(
        for (int l = 0; l < lanes; l++) (void) hipStreamSynchronize(ls[l]);
        for (int g = 0; g < (int) plan.units.size() && rc == KBE_OK; g++) {
            const PlanUnit& un = plan.units[g];
            float b = 0, r = 0, o = 0, c = 0;
            (void) hipEventElapsedTime(&b, ev_start, ev_begin[g]); (void) hipEventElapsedTime(&r, ev_start, ev_ready[g]);
            (void) hipEventElapsedTime(&o, ev_start, ev_gate[g]); (void) hipEventElapsedTime(&c, ev_start, ev_copied[g]);
            fprintf(stderr, "group %3d lane %d frames %3d..%3d: render %8.1f .. %8.1f us, gate open %8.1f, transfer ends %8.1f (%.1f GB/s from the gate)\n", g, un.lane,
                    un.first, un.first + un.count - 1, b * 1e3, r * 1e3, o * 1e3, c * 1e3, (double) un.count * fb / ((c - o) * 1e6));
        })
    }
};
}  // namespace

namespace kbe {

// what the call keeps in the module's own types (VideoHandoff::hidden holds it)
struct VideoHandoff::Hidden {
    SdmaCall sdma;
    DeliverCtl* ctl_turns = nullptr;    // the turn counter in `stage`, where the transfers take turns
    VideoTrace trace;
};
static_assert(sizeof(VideoHandoff::Hidden) <= sizeof(VideoHandoff::hidden) && alignof(VideoHandoff::Hidden) <= 16, "VideoHandoff::hidden holds a Hidden");

VideoHandoff::VideoHandoff() : hid(new (hidden) Hidden) {}
VideoHandoff::~VideoHandoff() { hid->~Hidden(); }

int VideoHandoff::open(const HandoffIn& in)
{
    static_cast<HandoffIn&>(*this) = in;
    n_ev = 0; ok = true;
    for (int l = 0; l < KBE_MAX_LANES; l++) lane_fin[l] = nullptr;
    // where do the frames go?  (a pointer the runtime does not know is taken for device memory, as before)
    host_dev = nullptr;
    if (batch <= 0) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, host_out) == hipSuccess && attr.type == hipMemoryTypeHost) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, host_out, 0) != hipSuccess || !dp)
                return fail(KBE_E_INVALID, "kbe_render_video: host_out is host memory the device cannot address (pin it with hipHostMalloc / hipHostRegister)");
            host_dev = (uint8_t*) dp;
        } else {
            (void) hipGetLastError();           // unknown to the runtime: not an error here
        }
    }
    dest = batch > 0 ? VideoDest::RING : !host_dev ? VideoDest::HBM : batch == 0 ? VideoDest::PER_FRAME : VideoDest::GROUPS;
    slots = dest == VideoDest::HBM ? host_out : stage + (dest == VideoDest::RING ? layout.ring : layout.finished);
    // the hand-off's turn counter sits behind the frame buffers of `stage`, 256-byte aligned
    KBE_REQUIRE(((uintptr_t) stage & 255) == 0, "kbe_render_video: stage must be 256-byte aligned");
    if (host_dev && lanes > 1) {
        // the turn counter of the hand-off starts at 0 for every call (on `stream`, before the other lanes start)
        const hipError_t e = hipMemsetAsync(stage + layout.ctl, 0, sizeof(DeliverCtl), ls[0]);
        if (e != hipSuccess) return fail(KBE_E_LAUNCH, "kbe_render_video: hipMemsetAsync", e);
    }
    // (where the rendering binds, not the link, the transfers need no order: a lane that waits for its turn only idles)
    hid->ctl_turns = host_dev && lanes > 1 && !(flags & KBE_VIDEO_FREE_TRANSFERS) ? (DeliverCtl*) (stage + layout.ctl) : nullptr;
    // KBE_VIDEO_SDMA: the groups leave through an SDMA engine (above); whatever keeps HSA from it falls back to the runtime's
    // transfers, group by group.  (Opened behind the first group's launches: the queries cost the host 10-25 us, which would
    // otherwise sit in front of the video's first kernel.)
    sdma_asked = !(flags & KBE_VIDEO_SDMA);
    // how long a group may wait for its turn: the transfers of every other lane in front of it (a poll is ~1 us; the
    // link moves ~50 bytes per ns), three times over -- a fixed 4 ms was no margin for 16 frames of 2048^2 (3.8 ms each)
    const double group_us = (double) -batch * (double) layout.fb / 50.0e3;
    turn_polls = (int) fmin(fmax(3.0 * lanes * group_us, (double) DELIVER_MAX_POLLS), 1.0e6);
    return KBE_OK;
}

hipEvent_t VideoHandoff::make()
{
    hipEvent_t e = nullptr;
    if (n_ev >= MAX_EV || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { ok = false; return nullptr; }
    pool[n_ev++] = e;
    return e;
}

// whoever synchronises `stream` afterwards also sees every frame delivered and every other stream idle
void VideoHandoff::join()
{
    const hipStream_t cs = ls[0];
    for (int l = 1; l < lanes && ok; l++) { hipEvent_t e = make(); if (e) { (void) hipEventRecord(e, ls[l]); (void) hipStreamWaitEvent(cs, e, 0); } }
    if (dest == VideoDest::RING && dc != cs && ok) { hipEvent_t e = make(); if (e) { (void) hipEventRecord(e, dc); (void) hipStreamWaitEvent(cs, e, 0); } }
}

int VideoHandoff::start(const VideoPlan& plan)
{
    const hipStream_t cs = ls[0];
    const bool ringed = dest == VideoDest::RING;
    hipEvent_t start = lanes > 1 || (ringed && dc != cs) ? make() : nullptr;
    // the other streams start once everything enqueued on `stream` so far (the cloud) is done
    if (start && ok) {
        (void) hipEventRecord(start, cs);
        for (int l = 1; l < lanes; l++) (void) hipStreamWaitEvent(ls[l], start, 0);
        if (ringed && dc != cs) (void) hipStreamWaitEvent(dc, start, 0);
    }
    for (int h = 0; h < 2 && ringed; h++) {
        copied[h] = make();
        for (int l = 0; l < lanes; l++) rendered[h][l] = ls[l] != dc ? make() : nullptr;
    }
    if (dest == VideoDest::GROUPS) hid->trace.start((int) plan.units.size(), cs);
    return ok ? KBE_OK : fail(KBE_E_LAUNCH, "kbe_render_video: hipEventCreate");      // (the call still runs to finish())
}

// ---- the hand-off, by destination (HBM: none).  PER_FRAME: k_deliver behind every frame in the lane's own stream; GROUPS: a
// transfer group rendered by ONE lane into its slots leaves through an SDMA engine, or with one runtime transfer (hipMemcpyAsync)
// between a gate kernel that waits for the turn and one that passes it on; RING: a half is copied to the host with ONE runtime
// transfer on the copy stream while the other half is being rendered, cross-stream events per half, not per frame.

// wait until the unit's slots are free
void VideoHandoff::before(int u, const PlanUnit& un)
{
    if (dest == VideoDest::GROUPS) {
        hid->trace.begin(u, ls[un.lane]);
        // (SDMA: the lane's slots hold the group it sent last -- until that has left.  Two sets of slots per lane, so that a
        // lane renders its next group while its last one leaves, measured SLOWER: 14.2 k instead of 14.6 k frames/s for 20
        // frames, 15.9 k instead of 16.6 k for 75 -- a lane then renders the group after next while the other lane still
        // renders the group the engine waits for)
        if (lane_fin[un.lane]) hipLaunchKernelGGL(k_signal_wait, dim3(1), dim3(64), 0, ls[un.lane], lane_fin[un.lane], sdma_pool().wait_ticks, sdma_pool().gave_up);
        lane_fin[un.lane] = nullptr;
    } else if (dest == VideoDest::RING && u >= 2) {
        for (int l = 0; l < lanes; l++) if (ls[l] != dc) (void) hipStreamWaitEvent(ls[l], copied[u & 1], 0);    // the half is free again
    }
}

// a transfer group: its frames leave through the engine or the runtime's transfer, the lanes taking turns on the link
int VideoHandoff::send_group(int u, const PlanUnit& un, const VideoPlan& plan)
{
    SdmaCall& sdma = hid->sdma;
    VideoTrace& trace = hid->trace;
    DeliverCtl* const ctl_turns = hid->ctl_turns;
    const size_t fb = layout.fb;
    const hipStream_t s = ls[un.lane];
    uint8_t* const base = stage + layout.finished + (size_t) un.lane * layout.fin * fb;
    const size_t bytes = (size_t) un.count * fb;
    trace.ready(u, s);
    if (!sdma_asked) { sdma_asked = true; (void) sdma_open(sdma, stage, host_out); }
    // the engine takes the copies in order: no turns -- while it takes them (a copy it refuses sends the rest of the video
    // through the runtime's transfers, which take turns again: ADVICE r5)
    DeliverCtl* ctl = sdma.ok ? nullptr : ctl_turns;
    if (ctl) hipLaunchKernelGGL(k_turn, dim3(1), dim3(64), 0, s, ctl, 0, turn_polls);
    trace.gate(u, s);
    bool sent = false;
    if (sdma.ok) {
        SdmaPair p;
        const bool paired = sdma_pair(sdma, p);
        if (paired && hsa_amd_memory_async_copy_on_engine(host_out + (size_t) un.first * fb, sdma.cpu, base, sdma.gpu, bytes, 1, &p.dep, p.fin,
                                                          sdma.engine, true) == HSA_STATUS_SUCCESS) {
            // the copy is on the engine and waits for its release: from here on an error must go through sdma_abort
            const bool inject = (flags & KBE_VIDEO_INJECT_FAULT) && u == (plan.units.size() > 1 ? 1 : 0);
            if (!inject) hipLaunchKernelGGL(k_signal_release, dim3(1), dim3(64), 0, s, p.dep_value);
            const hipError_t le = inject ? hipErrorLaunchFailure : hipGetLastError();
            if (le != hipSuccess) return fail(KBE_E_LAUNCH, inject ? "kbe_render_video: injected hand-off fault (KBE_VIDEO_INJECT_FAULT)" : "kbe_render_video/release", le);
            sdma.used.back().released = true;
            lane_fin[un.lane] = p.fin_value;
            sent = true;
        } else {
            // this group and the rest: the runtime's transfers (the pair, if there is one, was never handed to the engine: idle again)
            if (paired) { std::lock_guard<std::mutex> lock(sdma_pool().mu); sdma_pool().idle.push_back(sdma.used.back()); sdma.used.pop_back(); }
            sdma.ok = false;
            if (ctl_turns && !ctl) { ctl = ctl_turns; hipLaunchKernelGGL(k_turn, dim3(1), dim3(64), 0, s, ctl, 0, turn_polls); }
        }
    }
    const hipError_t e = sent ? hipSuccess : hipMemcpyAsync(host_out + (size_t) un.first * fb, base, bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return fail(KBE_E_LAUNCH, "kbe_render_video: hipMemcpyAsync", e);
    trace.copied(u, s);
    if (ctl) hipLaunchKernelGGL(k_turn, dim3(1), dim3(64), 0, s, ctl, 1, 0);
    const int rc = launched("kbe_render_video/turn");
    trace.sent(u, un);
    return rc;
}

// send the unit after its launches
int VideoHandoff::after(int u, const PlanUnit& un, const VideoPlan& plan)
{
    const size_t fb = layout.fb;
    switch (dest) {
    case VideoDest::PER_FRAME:
        hipLaunchKernelGGL(k_deliver, dim3(DELIVER_BLOCKS), dim3(DELIVER_THREADS), 0, ls[un.lane], slot(plan.frames[plan.launches[un.launch0].first]),
                           host_dev + (size_t) un.first * fb, fb, hid->ctl_turns, (uint32_t) un.first);
        return launched("kbe_render_video/deliver");
    case VideoDest::GROUPS: return send_group(u, un, plan);
    case VideoDest::RING: {
        const int h = u & 1;
        for (int l = 0; l < lanes; l++)
            if (ls[l] != dc) { (void) hipEventRecord(rendered[h][l], ls[l]); (void) hipStreamWaitEvent(dc, rendered[h][l], 0); }    // (same stream: ordered anyway)
        const hipError_t e = hipMemcpyAsync(host_out + (size_t) un.first * fb, stage + layout.ring + (size_t) h * batch * fb, (size_t) un.count * fb, hipMemcpyDeviceToHost, dc);
        if (e != hipSuccess) return fail(KBE_E_LAUNCH, "kbe_render_video: hipMemcpyAsync", e);
        (void) hipEventRecord(copied[h], dc);
        return KBE_OK;
    }
    default: return KBE_OK;             // HBM: the last kernel of every frame stored straight into host_out
    }
}

int VideoHandoff::finish(int rc, const VideoPlan& plan)
{
    // drain: (SDMA) a lane is done when its last group has left -- whoever waits for the lanes (join) waits for the frames
    for (int l = 0; l < lanes; l++)
        if (lane_fin[l] && rc == KBE_OK)            // (KBE_VIDEO_INJECT_TIMEOUT: one tick of patience -- the give-up path, for its test)
            hipLaunchKernelGGL(k_signal_wait, dim3(1), dim3(64), 0, ls[l], lane_fin[l], (flags & KBE_VIDEO_INJECT_TIMEOUT) ? 1ull : sdma_pool().wait_ticks, sdma_pool().gave_up);
    if (dest == VideoDest::GROUPS) hid->trace.finish(plan, ls, lanes, layout.fb, rc);
    if (rc != KBE_OK) sdma_abort(hid->sdma, ls, lanes);  // no copy of a failed call outlives it, none keeps waiting for its release
    join();
    sdma_close(hid->sdma, ls[0]);
    for (int k = 0; k < n_ev; k++) (void) hipEventDestroy(pool[k]);
    if (rc == KBE_OK && !ok) rc = fail(KBE_E_LAUNCH, "kbe_render_video: hipEventCreate");
    return rc;
}

}  // namespace kbe

extern "C" {

int kbe_video_handoff_status(void)
{
    SdmaPool& pool = sdma_pool();
    std::unique_lock<std::mutex> lock(pool.mu);
    // the word: 0 = nothing happened, 1 = a polling kernel gave up (not yet reported), 2 = reported -- the engine stays off either way
    // (sdma_open looks for != 0), but the error is this call's to report ONCE: the videos after it leave through the runtime's transfers
    // and are complete, their callers must not be told otherwise
    if (!pool.gave_up || __atomic_load_n(pool.gave_up, __ATOMIC_ACQUIRE) != 1) return KBE_OK;
    __atomic_store_n(pool.gave_up, 2, __ATOMIC_RELEASE);
    pool.state = -1;                                    // no more copies through the engine
    // the copies of calls that are still on record may yet complete: wait for them here, so that the caller may free its buffers
    std::vector<SdmaGeneration> gens;
    gens.swap(pool.running);
    lock.unlock();
    const auto t0 = std::chrono::steady_clock::now();
    for (SdmaGeneration& g : gens) {
        for (SdmaPair& p : g.pairs)
            while (hsa_signal_load_scacquire(p.fin) > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < KBE_SDMA_WAIT_SECONDS)
                std::this_thread::sleep_for(std::chrono::microseconds(50));
        (void) hipEventDestroy(g.done);                 // (their signals are never reused)
    }
    return fail(KBE_E_LAUNCH, "kbe_render_video: an SDMA hand-off gave up waiting for its engine -- the frames of that video are not all in host memory; the engine is not used again");
}

}  // extern "C"
