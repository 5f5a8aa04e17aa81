"""The shape of one ``kbe_render_video`` call, decided on plain values: the Python twin of ``csrc/kbe_video_plan.h``.

Nothing here touches the GPU, the library or the environment: ``_native.video_switches`` reads the environment once
per call into a :class:`Switches` record, ``HipKernels.render_video`` picks the lanes, and :func:`call_shape` makes of
them what the call passes -- lanes, batch, frames per launch, flags, route, scratch sets.  ``tests/test_host_logic.py``
drives it without a GPU.
"""
from collections import namedtuple

# the flag bits of kbe_render_video and the build bits of the one-frame / group entries, as include/kbe.h names them
# (tests/test_capi.py compares each with the header)
KBE_VIDEO_FILL_DIST = 1
KBE_VIDEO_FREE_TRANSFERS = 8
KBE_VIDEO_EVEN_GROUPS = 16
KBE_VIDEO_NO_AHEAD = 512
KBE_VIDEO_FAST_RAMP = 1024
KBE_VIDEO_FUSED_LEAN = 2048
KBE_VIDEO_FUSED_ROOMY = 4096
KBE_VIDEO_SDMA = 8192
KBE_VIDEO_INJECT_FAULT = 32768
KBE_VIDEO_INJECT_TIMEOUT = 65536
KBE_STAGE_PROJECT = 1
KBE_STAGE_FUSED_LEAN = 1024
KBE_STAGE_FUSED_ROOMY = 2048


def KBE_VIDEO_FILL_GROUP(n):
    """n = 1..4 frames per launch (either route)."""
    return (n - 1) << 1


def KBE_VIDEO_GROUP(n):
    """n = 1..12 frames per launch of the fused route."""
    return (n - 1) << 5


FUSED_DENSE = 1.5                # "denser than the raster" from here on: delivered to host memory such a video takes three frames per launch on every lane (two until round 6)
FUSED_HOST_GROUP = 12  # frames per launch of the fused scatter when the frames are delivered to host memory (KBE_FILL_GROUP overrides): as many as a
                       # launch's 4 KB of kernel arguments hold.  A launch alone on a stream costs ~5 us besides its frames (ramp and tail: 8 / 12
                       # frames per launch 16.5 / 16.1 us per frame), and delivered to host memory -- the link binds -- a video runs at the same rate
                       # with 8 or 12 (17.4-17.6 k frames/s, --steps 75 16.1-16.3 k, --steps 20 13.8-13.9 k either way: tools/batches/gpu_r04_group12.sh)
DEFAULT_FILL_GROUP = 4 # frames a lane fills per launch when the table-driven fill is on (env KBE_FILL_GROUP, 1..4)
DEFAULT_HOST_LANES = 2 # of the lanes, those used when the frames are delivered to pinned host memory AND the link binds (host_lanes below)
LINK_BYTES_PER_US = 53.0e3     # what the PCIe link moves for this loop (measured: 53-54.5 GB/s of the 63 GB/s Gen5 x16)
MAX_BATCH = 64         # the staging buffers grow with |batch| (lanes * (4 + G) frames): never more frames per transfer than this

# The environment switches of one video call, parsed (`_native.video_switches` is where they are read and listed).
Switches = namedtuple('Switches', 'fill_dist fill_group host_lanes delivery_batch fast_ramp free_transfers even_groups no_ahead build_bits '
                                  'sdma inject_fault inject_timeout scratch_budget_mb')
# what every switch is when its variable is unset
DEFAULTS = Switches(fill_dist=None, fill_group=None, host_lanes=None, delivery_batch=0, fast_ramp=False, free_transfers=None, even_groups=False,
                    no_ahead=False, build_bits=0, sdma=True, inject_fault=False, inject_timeout=False, scratch_budget_mb=None)

# lanes, batch, flags: kbe_render_video's arguments; group: frames per launch; fused: the route; sets: scratch sets the call renders on
CallShape = namedtuple('CallShape', 'lanes batch group flags fused sets')


def lanes_for_delivery(lanes, render_us, frame_bytes):
    """Two lanes where the link binds (it needs 1.5 x longer per frame than the rendering), all lanes elsewhere."""
    link_us = frame_bytes / LINK_BYTES_PER_US
    return min(lanes, DEFAULT_HOST_LANES) if link_us > 1.5 * render_us else lanes


def transfer_group(n_frames, lanes, launch_group, fast_ramp=False):
    """-(frames per transfer group) of a delivered video of n_frames on `lanes` lanes (kbe_render_video's batch < 0; the first groups
    ramp 1, 2, 4, ...: include/kbe.h).  Two lanes -- the link binds: groups of up to 32 frames (16 -> 32: 17.3 -> 17.5 k frames/s), a quarter of
    the video between 64 and 128 frames, 16 below.  More lanes -- the rendering binds, not the link (delivery_lanes): a
    lane then waits for nothing but its own last transfer, and what a video loses is its END -- the lanes' last groups leave one after
    the other when nothing is left to render, and groups of 32 deal the frames unevenly to four lanes: a transfer group is what ONE
    scatter launch renders (`launch_group`).  Measured (tools/batches/gpu_r05_dolly_batch.sh, profiles/r05_transfer_groups.txt): bench --dolly,
    256 frames, k frames/s delivered with groups of up to 32 / 16 / 12 / 8 frames 10.2 / 10.7 / 10.7 / 11.4 (left in HBM: 13.0);
    configs[4], 64 frames, groups of 32 / 2: 2.2 / 3.0 k."""
    if lanes > DEFAULT_HOST_LANES:
        return -max(1, int(launch_group))
    # (the ramp is never cut below 16: until late in round 5 a short video's cap was n / 4 alone -- "small enough for each lane to have two
    # groups of full size", a rule from the blit hand-off's days; with the SDMA engine a transfer fewer is worth more: tools/batches/gpu_r05_short_batch.sh,
    # k frames/s delivered with the old cap / 8 / 16: 16 frames 13.8-13.9 / 14.3 / 14.3, 20 frames 14.8 / 14.9 / 14.9, 30 frames 15.5 / 15.4 / 15.65; 40, 75: equal)
    return -max(1, min(32, max(n_frames // (2 * lanes), 16, (n_frames + 1) // 2 if fast_ramp else 0)))


def host_lanes(lanes, n_points, W, H, frame_bytes, forced=None):
    """The a-priori estimate (HipKernels.delivery_lanes measures instead, once per cloud, when the video is long enough).
    Lanes of the frame loop when the frames go to pinned host memory (`forced`, env KBE_HOST_LANES, overrides).  Where the PCIe
    link binds, two lanes ping-pong best (one renders its next group while the other's leaves: 59.1 us per 1024^2 frame of
    the bench against 60.7 with four and 84.8 with three); where the rendering binds every lane helps (measured, 2 -> 4
    lanes: 512^2 25.5 -> 18.8 us, dolly 260 -> 155, raw cloud 64 -> 61, 2048^2 raw 305 -> 276, 2048^2 from 16.8 M points
    427 -> 386).  Which it is, from what is known before the first frame: the link needs frame_bytes / 53 GB/s per frame; a
    frame of an inpainted cloud (more points than pixels: few holes to fill) renders in about 13.5 us per million points
    + 12 us per megapixel with four lanes, and never in less than the ~14 us its four launches take; a cloud without
    appended points leaves holes whose fill dominates (rendering binds).  The link binds when it needs 1.5 x longer."""
    if forced is not None:
        return min(lanes, max(1, forced))
    link_us = frame_bytes / LINK_BYTES_PER_US
    render_us = max(14.0, 13.5e-6 * n_points + 12.0e-6 * W * H)
    link_bound = n_points > W * H and link_us > 1.5 * render_us
    return min(lanes, DEFAULT_HOST_LANES) if link_bound else lanes


def fills_with_tables(N, W, H, zooms_out, sw):
    """KBE_VIDEO_FILL_DIST, the table-driven hole fill: for videos whose frames have hundreds of thousands of holes -- a
    cloud without appended points (no inpainting) seen by a camera that zooms out (a dolly zoom lowers the focal length:
    the image shrinks into an empty border).  Measured, us per frame without / with: dolly 300 / 129 at 1024^2, 77 / 63
    at 512^2 -- but a raw cloud on the ordinary camera path 35.2 / 37.8, 2048^2 139 / 151 (two more launches per frame
    that find few holes).  KBE_FILL_DIST=1 / 0 forces it on / off."""
    return bool(N <= W * H and zooms_out) if sw.fill_dist is None else sw.fill_dist


def frames_per_launch(N, W, H, fused, fill_dist, batch, to_host, sw):
    """KBE_VIDEO_FILL_GROUP(n) / KBE_VIDEO_GROUP(n): a lane renders n frames into n scratch sets, every launch taking all n.  A launch on its
    own is bound by its ramp and its tail as much as by its work (the fused scatter of a 1024^2 frame: 35 us alone, 27 /
    23 per frame with 2 / 4 frames per launch), so frames left in HBM take 27.5 / 25.3 / 26.7 us with n = 1 / 2 / 4 on
    four lanes (the lanes fill the same gaps), and where the PCIe link binds (frames delivered to host memory: 59 us
    per frame whatever n) n = 4 leaves the most of the chip idle.  Small frames are bound by their launches: 4 up to
    576^2.  KBE_FILL_GROUP overrides.
    The route: the cloud's (prepare_cloud)."""
    # (until round 5 a zoom-out took the bucket route: the density of the points on the shrinking image grows along the video, the fused
    # route's candidate lists of 512 sub-blocks overflowed and it lost 147 : 97 us per frame.  With lists of 2048 it wins: 82 against
    # 90 us per 1024^2 dolly frame left in HBM, 21.8 against 23.5 at 512^2 -- profiles/r05_dolly_routes.txt.  KBE_FUSED=0 still forces the other.)
    if sw.fill_group is not None:
        group = max(1, min(12 if fused else 4, sw.fill_group))
    elif fill_dist:
        # the table-driven fill: launches bound by their own chains of look-ups -- four frames per fill launch; the fused scatter in
        # front of them takes eight (measured, us per dolly frame left in HBM / k frames/s delivered with 4 / 8 / 12: 82.1 / 80.4 / 79.7, 9.6 / 9.9 / 9.8)
        group = 8 if fused else DEFAULT_FILL_GROUP
    elif fused:
        # eight where the link binds (the rendering then only has to stay out of the transfers' way: the fewer, larger
        # launches the better), four for frames left in HBM on four lanes -- since a group's tile launch also makes the next
        # group's placements (one scatter launch per group) four frames per launch are as good as or better than two at every
        # size (measured, us per frame left in HBM with 2 / 4 / 8 frames per launch: 640^2 12.2 / 11.3 / 11.4, 896^2 20.3 / 20.9 / 21.3,
        # 1024^2 25.5 / 24.9 / 25.0, 1280^2 41.4 / 40.5 / 41.2, 1536^2 59.3 / 58.4 / 58.5; with a placement launch per group, round
        # 3's first half: 1024^2 25.3 / 26.7; the bucket route: 13.7, 18.8, 25.5, 29.4, 51.7, 72.8)
        group = FUSED_HOST_GROUP if to_host else 4
        if N > FUSED_DENSE * W * H:              # (left in HBM too since round 6: four per launch was the slowest of 2 / 3 / 4 there)
            # a cloud much denser than the raster is bound by its rendering, not by the link: few frames per launch on every lane.  Round 4
            # (blit hand-off: long launches next to another lane's copy kernel slowed each other), 16.8 M points at 2048^2, us per
            # delivered frame with 8 / 4 / 2 frames per launch on four lanes: 446 / 422 / 395.  Round 6, SDMA hand-off, frames/s delivered /
            # left in HBM with 2 / 3 / 4 / 6 / 8: 2 948 / 3 234, 2 941 / 3 246, 2 707 / 3 141, 2 598 / 2 999, 2 390 / 2 974 -- and the launch
            # alone on a stream 289.5 / 273.8 / 269.1 / 265.6 / 263.7 us per frame (its tail amortised): three is as fast as two for the
            # video and 5 % faster per launch (tools/batches/gpu_r06_config4_groups.sh, profiles/r06_config4_groups.txt)
            group = 3
    else:
        # the bucket route (measured, us per frame with 1 / 2 / 4 frames per launch: 256^2 13.3 / 9.8 / 6.2, 512^2 13.7 / 9.8 /
        # 8.6, 640^2 15.1 / 12.8 / 13.1, 768^2 19.1 / 16.4 / 17.4, 896^2 24.8 / 23.8 / 24.3, 1024^2 28.9 / 30.6 / 30.9)
        group = 4 if W * H <= 576 * 576 else (2 if W * H <= 900 * 900 else 1)
    if not (batch is None or batch <= 0):
        group = 1                                # the staged ring: one frame per launch
    return group if fused else min(group, 4)


def launch_flags(fill_dist, group):
    """The two fields of kbe_render_video's flags that the frames per launch and the fill decide."""
    return (KBE_VIDEO_FILL_DIST if fill_dist else 0) | (KBE_VIDEO_FILL_GROUP(group) if group <= 4 else KBE_VIDEO_GROUP(group))


def call_shape(N, W, H, fused, n_frames, zooms_out, to_host, batch, lanes, sw, held_sets, budget_sets):
    """What one video call passes to kbe_render_video, as a :class:`CallShape`.

    N, W, H, fused: the cloud (points, frame size, route).  n_frames, zooms_out, to_host: the video (to_host: the frames go to
    pinned host memory; else they stay in HBM).  batch: the caller's (None: by the switches and `transfer_group`; taken as given
    otherwise, 0 = per-frame delivery).  lanes: the lanes already chosen (all of the cloud's for frames left in HBM,
    HipKernels.delivery_lanes else).  sw: the :class:`Switches`.  held_sets: scratch sets the cloud's group scratch already
    holds; budget_sets(): how many it may hold -- only called when those held do not do or KBE_SCRATCH_BUDGET_MB is set (it
    reads the device's free memory, ~10 us of a call)."""
    fill_dist = fills_with_tables(N, W, H, zooms_out, sw)
    # The hand-off (include/kbe.h): < 0 = groups of -batch frames per lane, one transfer each, the lanes taking turns on the
    # link (default); 0 = per frame by a copy kernel; > 0 = round 1's staged ring.
    if not to_host:
        batch = 0
    elif batch is None:
        # how many frames a transfer group may hold: transfer_group (the first groups ramp 1, 2, 4, 8, 16: include/kbe.h)
        # (KBE_RAMP=fast: groups of 1, 3, 7, 15, 31, ... frames, capped at half the video -- two transfers fewer than 1, 2, 4, 8, ...
        # for a 20- or a 75-frame video.  Measured, round 4 (profiles/r04_short_videos.txt): no gain -- 20 frames 14.05 against
        # 13.93 k frames/s, 75 frames 16.05 against 16.21 k: the larger groups render next to the other lane's transfer, whose
        # blit kernel's PCIe-bound stores slow them.  Not the default.)
        launch_group = frames_per_launch(N, W, H, fused, fill_dist, None, True, sw) if lanes > DEFAULT_HOST_LANES else 0
        batch = sw.delivery_batch or transfer_group(n_frames, lanes, launch_group, sw.fast_ramp)
    batch = int(batch)
    cap = min(max(n_frames, 1), MAX_BATCH)       # never more frames per transfer than the video has
    batch = -min(-batch, cap) if batch < 0 else min(batch, cap)
    group = frames_per_launch(N, W, H, fused, fill_dist, batch, to_host, sw)
    if group > 1 and (held_sets < group * lanes or sw.scratch_budget_mb is not None):
        # n scratch sets per lane in use, allocated on first use -- 224 MB each at 1024^2, 0.9 GB at 2048^2 (most of it the
        # bucket / spill area): a launch shape that would take more than the budget (KBE_SCRATCH_BUDGET_MB, default half of
        # what is free, never less than one set per lane) falls back to fewer frames per launch.
        # (`batch` stays what the uncut shape gave it -- on more than two lanes a transfer group then spans several launches: as
        # the loop has always done, kept as it is)
        max_sets = budget_sets()
        while group > 1 and group * lanes > max_sets:
            group = max(1, group // 2)
    flags = launch_flags(fill_dist, group) | sw.build_bits            # KBE_FUSED_CAP: KBE_VIDEO_FUSED_LEAN / _ROOMY
    # KBE_VIDEO_FREE_TRANSFERS: videos that fill with the tables are bound by their rendering (the link is half idle), and
    # a lane waiting for its turn on the link only idles: bench --dolly 8.1 k frames/s delivered with turns, 9.1 k without
    # (512^2 and 2048^2 frames, whose transfers fill the link to 70 %, keep the turns: 57 vs 53 k, 2.65 vs 2.03 k)
    if to_host and (fill_dist if sw.free_transfers is None else sw.free_transfers):
        flags |= KBE_VIDEO_FREE_TRANSFERS
    if sw.even_groups:                           # (dev) transfer groups of one size instead of the ramp 1, 2, 4, ...
        flags |= KBE_VIDEO_EVEN_GROUPS
    if sw.fast_ramp:                             # transfer groups of 1, 3, 7, 15, ... frames
        flags |= KBE_VIDEO_FAST_RAMP
    if sw.no_ahead:                              # every group of the fused route keeps its own placement launch
        flags |= KBE_VIDEO_NO_AHEAD
    if to_host and batch < 0 and sw.sdma:
        flags |= KBE_VIDEO_SDMA
        if sw.inject_fault:                      # (test hook: tests/test_hip_parity.py)
            flags |= KBE_VIDEO_INJECT_FAULT
        if sw.inject_timeout:                    # (test hook)
            flags |= KBE_VIDEO_INJECT_TIMEOUT
    return CallShape(lanes=lanes, batch=batch, group=group, flags=flags, fused=fused, sets=group * lanes)
