#!/usr/bin/env python3
"""What the 4:2:0 planes cost and save (yuv.py, kbe_yuv420_u8), SIZE x SIZE frames:
  kernel:  HIP events around kbe_yuv420_u8 alone -- the raw entry on frames and payloads that lie in HBM already, nothing allocated --, FRAMES_IN_HBM
           frames, a warm-up and then the median of 10 calls.  Its traffic is 4.5 W H bytes a frame, 3 read and 1.5 written, and its rate is that
           traffic over the time.  In the same run, taking turns with it, a device-to-device copy_ whose traffic is as many bytes (it reads
           half of them and writes half); the kernel's rate is reported as a share of that copy's rate: the copy is the yardstick, no fixed
           number.  (At 12 frames of 1024 x 1024 the whole traffic is smaller than the chip's last-level cache, for the kernel and the copy alike.)
  route, on the bench's scene (bench.build_scene, inpainted cloud), arms taking turns in this one process, wall clock around calls that end
  with the FRAMES frames in host memory:
    rgb          render_frames(cameras, oc, crop): the video as 3-byte pixels, fetched while it is rendered;
    planes       render_frames(cameras, oc, crop, keep_on_device=True), yuv.convert, one fetch of the payloads into a pinned buffer that is
                 kept across the calls: half the bytes cross the link, but only after the last frame is rendered;
    planes_fresh the same with a pinned buffer allocated by every call, as yuv.write_y4m does it.
One JSON line on stdout and in --out (default profiles/yuv.json).  Needs a GPU: without one it exits with an error."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def pointers(t):
    return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(t, scale=1.0):
    return {'median': scale * float(np.median(t)), 'min': scale * min(t), 'max': scale * max(t), 'calls': len(t)}


def kernel_rate(size, n):
    from ken_burns_effect_amd import _native, yuv
    frames = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, device='cuda')
    out = torch.empty(n, yuv.frame_bytes(size, size), dtype=torch.uint8, device='cuda')
    traffic = n * (3 * size * size + yuv.frame_bytes(size, size))
    source, target = torch.randint(0, 256, (traffic // 2,), dtype=torch.uint8, device='cuda'), torch.empty(traffic // 2, dtype=torch.uint8, device='cuda')
    tables = pointers(frames), pointers(out)
    arms = {'kernel': lambda: yuv._call('kbe_yuv420_u8', tables[0], n, size, size, 3 * size, tables[1], 0, _native._stream()),
            'copy': lambda: target.copy_(source)}
    ms = {name: [] for name in arms}
    for turn in range(13):                                        # three turns of warm-up, then ten, the two taking turns
        for name, arm in arms.items():
            t = timed(arm)
            if turn >= 3:
                ms[name].append(t)
    assert torch.equal(out[:1], yuv.convert(frames[:1]))
    rate = {name: traffic / (1e6 * float(np.median(t))) for name, t in ms.items()}               # bytes / (1e-3 s) / 1e9
    return {'frames_in_hbm': n, 'traffic_bytes_per_call': traffic, 'kernel_ms': spread(ms['kernel']), 'copy_ms': spread(ms['copy']),
            'kernel_GB_per_s': rate['kernel'], 'copy_GB_per_s': rate['copy'], 'kernel_share_of_the_copys_rate': rate['kernel'] / rate['copy']}


def route_times(size, n, seconds):
    import bench
    from ken_burns_effect_amd import common, synthetic, yuv
    ofrom, oto = synthetic.default_windows(size, size, False)
    settings = {'dblSteps': [i / (n - 1) for i in range(n)], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False}
    oc = bench.build_scene(size, torch.device('cuda:0'), True, dict(settings, boolInpaint=True))
    cameras, crop = common.frame_cameras(settings, oc), common.crop_size(settings)
    kept = torch.empty(n, yuv.frame_bytes(size, size), dtype=torch.uint8, pin_memory=True)

    def planes(host=None):
        payloads = yuv.convert(common.render_frames(cameras, oc, crop, keep_on_device=True))
        host = torch.empty(payloads.shape, dtype=torch.uint8, pin_memory=True) if host is None else host
        host.copy_(payloads, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return host.numpy()
    arms = {'rgb': lambda: common.render_frames(cameras, oc, crop), 'planes': lambda: planes(kept), 'planes_fresh': planes}
    shapes = {name: tuple(np.shape(arm())) for name, arm in arms.items()}           # warm-up, and what comes back
    assert shapes == {'rgb': (n, size, size, 3), 'planes': (n, yuv.frame_bytes(size, size)), 'planes_fresh': (n, yuv.frame_bytes(size, size))}, shapes
    times = {name: [] for name in arms}
    while True:                                                       # taking turns; an arm stops once it has its SECONDS and three calls
        wanted = [(name, arm) for name, arm in arms.items() if sum(times[name]) < seconds or len(times[name]) < 3]
        if not wanted:
            break
        for name, arm in wanted:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    found = {name + '_ms_per_video': spread(t, 1e3) for name, t in times.items()}
    found['planes_over_rgb'] = found['planes_ms_per_video']['median'] / found['rgb_ms_per_video']['median']
    found['bytes_fetched'] = {'rgb': 3 * size * size * n, 'planes': yuv.frame_bytes(size, size) * n}
    found['points'], found['crop'] = int(oc['tensorInpaPoints'].shape[2]), list(crop)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=75)
    ap.add_argument('--frames-in-hbm', type=int, default=12)
    ap.add_argument('--seconds', type=float, default=2.0, help='per arm of the route, and at least three calls')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'yuv.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('yuv_time.py measures on a GPU, and there is none')
    line = dict(what='4:2:0 planes: kbe_yuv420_u8 alone beside a device-to-device copy of as much traffic, and a delivered video as RGB and as planes',
                size=args.size, frames=args.frames, gpu=torch.cuda.get_device_name(0), kernel=kernel_rate(args.size, args.frames_in_hbm),
                **route_times(args.size, args.frames, args.seconds))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
