#!/usr/bin/env python3
"""What motion blur costs (shutter.py, common.render_frames(shutter=...)), SIZE x SIZE frames:
  kernel:  HIP events around kbe_shutter_mean_u8 alone -- the raw entry on frames and outputs that lie in HBM already, nothing allocated --,
           OUTPUTS output frames of S = 2, 8 and 32 samples each, a warm-up and then the median of 10 calls.  Its traffic is (S + 1) * 3 W H
           bytes per output, read and written, and its rate is that traffic over the time.  In the same run, taking turns with it, a
           device-to-device copy_ whose traffic is as many bytes (it reads half of them and writes half); the kernel's rate is reported as
           a share of that copy's rate: the copy is the yardstick, no fixed number.  (At S = 2 the whole traffic is smaller than the chip's
           last-level cache, for the kernel and the copy alike.)
  route, on the bench's scene (bench.build_scene, inpainted cloud), arms taking turns in this one process, wall clock around calls that end
  with the FRAMES frames in host memory:
    plain        render_frames(cameras, oc, crop): the video without a shutter;
    shutter_S    render_frames(the FRAMES * S cameras of shutter.sample_steps, oc, crop, shutter=Shutter(0.5, S)), S = 2, 8 and 32.
One JSON line on stdout and in --out (default profiles/shutter.json).  Needs a GPU: without one it exits with an error."""
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

SAMPLES = (2, 8, 32)


def pointers(t):
    return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_rates(size, outputs):
    from ken_burns_effect_amd import _native, shutter
    found = {}
    for S in SAMPLES:
        frames = torch.randint(0, 256, (outputs * S, size, size, 3), dtype=torch.uint8, device='cuda')
        out = torch.empty(outputs, size, size, 3, dtype=torch.uint8, device='cuda')
        traffic = (S + 1) * 3 * size * size * outputs
        source, target = torch.randint(0, 256, (traffic // 2,), dtype=torch.uint8, device='cuda'), torch.empty(traffic // 2, dtype=torch.uint8, device='cuda')
        tables = pointers(frames), pointers(out)
        arms = {'kernel': lambda: shutter._call('kbe_shutter_mean_u8', tables[0], outputs, S, size, size, 3 * size, tables[1], 3 * size, _native._stream()),
                'copy': lambda: target.copy_(source)}
        ms = {name: [] for name in arms}
        for turn in range(13):                                    # three turns of warm-up, then ten, the two taking turns
            for name, arm in arms.items():
                t = timed(arm)
                if turn >= 3:
                    ms[name].append(t)
        assert torch.equal(out[:1], shutter.mean(frames[:S], S))
        rate = {name: traffic / (1e6 * float(np.median(t))) for name, t in ms.items()}           # bytes / (1e-3 s) / 1e9
        found['S_%d' % S] = {'outputs': outputs, 'traffic_bytes_per_call': traffic,
                             'kernel_ms': {'median': float(np.median(ms['kernel'])), 'min': min(ms['kernel']), 'max': max(ms['kernel']), 'calls': len(ms['kernel'])},
                             'copy_ms': {'median': float(np.median(ms['copy'])), 'min': min(ms['copy']), 'max': max(ms['copy']), 'calls': len(ms['copy'])},
                             'kernel_GB_per_s': rate['kernel'], 'copy_GB_per_s': rate['copy'], 'kernel_share_of_the_copys_rate': rate['kernel'] / rate['copy']}
        del frames, out, source, target
    return found


def route_times(size, n, seconds):
    import bench
    from ken_burns_effect_amd import common, shutter, synthetic
    ofrom, oto = synthetic.default_windows(size, size, False)
    settings = {'dblSteps': [i / (n - 1) for i in range(n)], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False}
    oc = bench.build_scene(size, torch.device('cuda:0'), True, dict(settings, boolInpaint=True))
    cameras, crop = common.frame_cameras(settings, oc), common.crop_size(settings)
    arms = {'plain': lambda: common.render_frames(cameras, oc, crop)}
    for S in SAMPLES:
        expanded = common.frame_cameras(dict(settings, dblSteps=shutter.sample_steps(settings['dblSteps'], 0.5, S)), oc)
        arms['shutter_%d' % S] = lambda expanded=expanded, S=S: common.render_frames(expanded, oc, crop, shutter=shutter.Shutter(0.5, S))
    shapes = {name: tuple(np.shape(arm())) for name, arm in arms.items()}           # warm-up, and what comes back
    assert all(shape == (n, size, size, 3) for shape in shapes.values()), shapes
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
    found = {name + '_ms_per_video': {'median': 1e3 * float(np.median(t)), 'min': 1e3 * min(t), 'max': 1e3 * max(t), 'calls': len(t)} for name, t in times.items()}
    found['points'], found['crop'] = int(oc['tensorInpaPoints'].shape[2]), list(crop)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=75)
    ap.add_argument('--outputs', type=int, default=12)
    ap.add_argument('--seconds', type=float, default=2.0, help='per arm of the route, and at least three calls')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shutter.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('shutter_time.py measures on a GPU, and there is none')
    line = dict(what='motion blur: kbe_shutter_mean_u8 alone beside a device-to-device copy of as much traffic, and a delivered video with and without a shutter',
                size=args.size, frames=args.frames, gpu=torch.cuda.get_device_name(0), kernel=kernel_rates(args.size, args.outputs),
                **route_times(args.size, args.frames, args.seconds))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
