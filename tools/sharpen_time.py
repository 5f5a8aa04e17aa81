#!/usr/bin/env python3
"""What output sharpening costs (sharpen.py), arms taking turns in this one process:
  kernel:  HIP events around the entry alone -- the raw entry on frames that lie in HBM already, nothing allocated --, FRAMES frames per call:
           SIZE x SIZE (1024) at sigma 1 (radius 3) and sigma 8 (radius 24), and 1920 x 1920 at sigma 1.5 (radius 5).  A sample is
           LAUNCHES = 10 calls back to back between two events, divided by 10; three turns of warm-up and then the median of 10 samples each.
           The entry reads a frame's 3 bytes per pixel and writes 3: that is its traffic (a tile's halo is read again by its neighbours,
           out of the caches; not counted), and its rate is that traffic over its time.  In the same turns, per case, a device-to-device
           copy_ of as many bytes (it reads half of them and writes half), and the lens blur kbe_dof_u8 on the same frames at a like radius:
           a constant depth at twice the focus depth, so that every pixel gathers a disc of the sharpening's radius -- capped at 16, the
           lens' own limit, for sigma 8.  Reported: every arm's median, minimum and maximum, the rates, the sharpening's share of its copy's
           rate, and the time per output pixel of the sharpening and of the lens blur.
  route:   wall clock, one synthetic photo of SIZE with seeded weights, one Pipeline: a delivered video of VIDEO_FRAMES frames with
           width=1920, enlarge=True, sharpen='1,1.5' against the same video without sharpen plus Pillow's UnsharpMask(1.5, 100, 0) of every
           returned frame on the host.
One JSON line on stdout and in --out (default profiles/sharpen.json).  Needs a GPU: without one it exits with an error."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def pointers(t):
    return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])


LAUNCHES = 10          # back-to-back calls between the two events of one sample
LENS_MAX_RADIUS = 16   # dof.MAX_RADIUS


def timed(call, launches=LAUNCHES):
    """Milliseconds per call: `launches` calls back to back between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def stats(ms):
    return {'median': float(np.median(ms)), 'min': min(ms), 'max': max(ms), 'calls': len(ms)}


def kernel_times(cases, frames):
    """cases: [(side, sigma)]."""
    from ken_burns_effect_amd import _native, dof, sharpen
    arms, traffic, pixels, radii = {}, {}, {}, {}
    for side, sigma in cases:
        tag = '%d_sigma_%g' % (side, sigma)
        request = sharpen.request((1, sigma), environment=False)
        R = request['radius']
        raw = torch.randint(0, 256, (frames, side, side, 3), dtype=torch.uint8, device='cuda')
        out = torch.empty_like(raw)
        blurred = torch.empty_like(raw)
        depth = torch.full((frames, side, side), 2.0, dtype=torch.float32, device='cuda')
        planes = (ctypes.c_void_p * frames)(*[depth[i].data_ptr() for i in range(frames)])
        focus = (ctypes.c_double * frames)(*[1.0] * frames)
        lens_radius = min(R, LENS_MAX_RADIUS)
        taps = (ctypes.c_uint16 * (R + 1))(*request['taps'])
        traffic['sharpen_' + tag] = traffic['copy_' + tag] = traffic['lens_' + tag] = 2 * 3 * frames * side * side
        pixels['sharpen_' + tag] = pixels['lens_' + tag] = frames * side * side
        radii[tag] = {'sharpen': R, 'lens': lens_radius}
        half = 3 * frames * side * side
        source, target = torch.randint(0, 256, (half,), dtype=torch.uint8, device='cuda'), torch.empty(half, dtype=torch.uint8, device='cuda')
        arms['sharpen_' + tag] = lambda sources=pointers(raw), targets=pointers(out), side=side, taps=taps, R=R, request=request: sharpen._call(
            'kbe_sharpen_u8', sources, frames, side, side, 3 * side, targets, 3 * side, taps, R, request['amount'], request['threshold'], _native._stream())
        arms['copy_' + tag] = lambda source=source, target=target: target.copy_(source)
        # (a depth of twice the focus depth: r = min(max_radius, round(aperture / 2)) for every pixel)
        arms['lens_' + tag] = lambda sources=pointers(raw), targets=pointers(blurred), side=side, planes=planes, focus=focus, lens_radius=lens_radius: dof._call(
            'kbe_dof_u8', sources, planes, frames, side, side, 3 * side, side, focus, 2.0 * lens_radius, LENS_MAX_RADIUS, targets, 3 * side, _native._stream())
        # the arm is the entry sharpen.apply_sharpen calls: one frame through both, the same bytes
        arms['sharpen_' + tag]()
        assert torch.equal(out[:1], sharpen.apply_sharpen(raw[:1].clone(), request))
        arms['lens_' + tag]()
        assert not torch.equal(blurred[:1], raw[:1])
    ms = {name: [] for name in arms}
    for turn in range(13):                                        # three turns of warm-up, then ten, the arms taking turns
        for name, arm in arms.items():
            t = timed(arm)
            if turn >= 3:
                ms[name].append(t)
    found = {name + '_ms': stats(t) for name, t in ms.items()}
    rate = {name: traffic[name] / (1e6 * found[name + '_ms']['median']) for name in arms}      # bytes / (1e-3 s) / 1e9
    found.update(frames=frames, radii=radii, launches_per_sample=LAUNCHES, traffic_bytes_per_call=traffic, GB_per_s=rate,
                 share_of_the_copys_rate={name: rate[name] / rate['copy_' + name[len('sharpen_'):]] for name in arms if name.startswith('sharpen_')},
                 ns_per_output_pixel={name: 1e6 * found[name + '_ms']['median'] / count for name, count in pixels.items()})
    return found


def route_times(size, frames, calls, wide, setting, sigma, percent):
    from PIL import Image, ImageFilter
    from ken_burns_effect_amd import kbe, slideshow, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    image = synthetic.make_rgbd(size, size, 0)[0]
    zoom = kbe.windows_for(size, size, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, device='cuda:0', steps=frames, miopen_find=False, width=wide, enlarge=True)
    mask = ImageFilter.UnsharpMask(radius=sigma, percent=percent, threshold=0)
    with tempfile.TemporaryDirectory() as tmp:
        def on_the_gpu():
            pipe.sharpen = setting
            return pipe(image, zoom, os.path.join(tmp, 'sharpened'))

        def on_the_host():
            pipe.sharpen = None
            return [np.asarray(Image.fromarray(f).filter(mask)) for f in pipe(image, zoom, os.path.join(tmp, 'plain'))]

        def neither():
            pipe.sharpen = None
            return pipe(image, zoom, os.path.join(tmp, 'plain'))
        arms = {'sharpen_on_the_gpu': on_the_gpu, 'plain_then_pillow': on_the_host, 'plain': neither}
        times, shapes = {name: [] for name in arms}, {}
        for turn in range(calls + 1):                             # one turn of warm-up
            for name, arm in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = arm()
                torch.cuda.synchronize()
                shapes[name] = [len(got)] + list(got[0].shape)
                if turn >= 1:
                    times[name].append(1e3 * (time.perf_counter() - t0))
    assert shapes['sharpen_on_the_gpu'] == shapes['plain_then_pillow'] == [frames, wide, wide, 3], shapes
    found = {name + '_ms': stats(t) for name, t in times.items()}
    found.update(photo_size=size, frames=frames, width=wide, sharpen=setting, jpeg=os.environ.get('KBE_JPEG', 'native'),
                 note='the first arm also writes its video from the sharpened frames; the second writes it from the plain ones and sharpens only the returned frames',
                 gpu_share_of_host=found['sharpen_on_the_gpu_ms']['median'] / found['plain_then_pillow_ms']['median'])
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--video-frames', type=int, default=75)
    ap.add_argument('--calls', type=int, default=3, help='per arm of the route, after one warm-up')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sharpen.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('sharpen_time.py measures on a GPU, and there is none')
    wide = 1920 * args.size // 1024
    line = dict(what='the unsharp mask: the entry alone at sigma 1 and 8 on the photo\'s size and at sigma 1.5 on frames 1920 wide, each beside a device-to-device copy of as much traffic '
                     'and the lens blur at a like radius; and a delivered video enlarged and sharpened on the GPU against the same video sharpened by Pillow on the host',
                size=args.size, gpu=torch.cuda.get_device_name(0), kernel=kernel_times([(args.size, 1.0), (args.size, 8.0), (wide, 1.5)], args.frames),
                route=route_times(args.size, args.video_frames, args.calls, wide, '1,1.5', 1.5, 100))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
