#!/usr/bin/env python3
"""What an enlargement costs (enlarge.py), arms taking turns in this one process:
  kernel:  HIP events around the entry alone -- the raw entry on frames that lie in HBM already, nothing allocated --, FRAMES raw frames of
           SIZE x SIZE per call, their centred crop of 0.9 SIZE (921 of 1024) enlarged to 1920 wide and, 4-fold, to 3684 wide.  A sample is
           LAUNCHES = 10 calls back to back between two events, divided by 10; three turns of warm-up and then the median of 10 samples each.
           The entry reads the crop's 3 bytes per pixel and writes the target's 3: that is its traffic (a tile's span is staged once per
           tile, so the rows and columns that neighbouring tiles share are read again, out of the caches; not counted), and its rate is
           that traffic over its time.  In the same turns, per target, a device-to-device copy_ of as many bytes (it reads half of them and
           writes half), and once the existing bilinear enlargement of the same crop to SIZE x SIZE, K.crop_resize_u8 frame by frame as the
           default route calls it.  Reported: every arm's median, minimum and maximum, the rates, the enlargements' shares of their copy's
           rate, and their time per output pixel beside the bilinear one's.
  route:   wall clock, one synthetic photo of SIZE with seeded weights, one Pipeline: a delivered video of VIDEO_FRAMES frames with
           width=1920, enlarge=True against the same video at full size plus Pillow's resize(BICUBIC) of every returned frame on the host.
One JSON line on stdout and in --out (default profiles/enlarge.json).  Needs a GPU: without one it exits with an error."""
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


def kernel_times(size, frames, widths):
    from ken_burns_effect_amd import _native, enlarge
    K = _native.kernels()
    crop = int(0.9 * size)
    raw = torch.randint(0, 256, (frames, size, size, 3), dtype=torch.uint8, device='cuda')
    sources = pointers(raw)
    arms, traffic = {}, {}
    for wide in widths:
        out = torch.empty(frames, wide, wide, 3, dtype=torch.uint8, device='cuda')
        traffic['enlarge_%d' % wide] = traffic['copy_%d' % wide] = 3 * frames * (crop * crop + wide * wide)
        half = traffic['copy_%d' % wide] // 2
        source, target = torch.randint(0, 256, (half,), dtype=torch.uint8, device='cuda'), torch.empty(half, dtype=torch.uint8, device='cuda')
        arms['enlarge_%d' % wide] = lambda out=out, targets=pointers(out), wide=wide: enlarge._call('kbe_enlarge_u8', sources, frames, size, size, 3 * size, crop, crop, targets, wide, wide,
                                                                                                     3 * wide, _native._stream())
        arms['copy_%d' % wide] = lambda source=source, target=target: target.copy_(source)
        # the arm is the entry enlarge.enlarge calls: one frame through both, the same bytes
        arms['enlarge_%d' % wide]()
        assert torch.equal(out[:1], enlarge.enlarge(raw[:1], (crop, crop), (wide, wide)))
    traffic['bilinear_to_%d' % size] = 3 * frames * (crop * crop + size * size)
    arms['bilinear_to_%d' % size] = lambda: [K.crop_resize_u8(raw[i], crop, crop) for i in range(frames)]
    ms = {name: [] for name in arms}
    for turn in range(13):                                        # three turns of warm-up, then ten, the arms taking turns
        for name, arm in arms.items():
            t = timed(arm)
            if turn >= 3:
                ms[name].append(t)
    found = {name + '_ms': stats(t) for name, t in ms.items()}
    rate = {name: traffic[name] / (1e6 * found[name + '_ms']['median']) for name in arms}      # bytes / (1e-3 s) / 1e9
    pixels = dict({'enlarge_%d' % wide: frames * wide * wide for wide in widths}, **{'bilinear_to_%d' % size: frames * size * size})
    found.update(frames=frames, crop=crop, launches_per_sample=LAUNCHES, traffic_bytes_per_call=traffic, GB_per_s=rate,
                 share_of_the_copys_rate={'enlarge_%d' % wide: rate['enlarge_%d' % wide] / rate['copy_%d' % wide] for wide in widths},
                 ns_per_output_pixel={name: 1e6 * found[name + '_ms']['median'] / count for name, count in pixels.items()})
    return found


def route_times(size, frames, calls, wide):
    from PIL import Image
    from ken_burns_effect_amd import kbe, slideshow, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    image = synthetic.make_rgbd(size, size, 0)[0]
    zoom = kbe.windows_for(size, size, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, device='cuda:0', steps=frames, miopen_find=False)
    with tempfile.TemporaryDirectory() as tmp:
        def enlarged():
            pipe.width, pipe.enlarge = wide, True
            return pipe(image, zoom, os.path.join(tmp, 'enlarged'))

        def on_the_host():
            pipe.width, pipe.enlarge = None, None
            return [np.asarray(Image.fromarray(f).resize((wide, wide), Image.BICUBIC)) for f in pipe(image, zoom, os.path.join(tmp, 'plain'))]
        arms = {'enlarge_on_the_gpu': enlarged, 'full_size_then_pillow': on_the_host}
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
    assert shapes['enlarge_on_the_gpu'] == shapes['full_size_then_pillow'] == [frames, wide, wide, 3], shapes
    found = {name + '_ms': stats(t) for name, t in times.items()}
    found.update(photo_size=size, frames=frames, width=wide, jpeg=os.environ.get('KBE_JPEG', 'native'),
                 note='the first arm also writes its video at the enlarged size; the second writes it at the photo\'s size and enlarges only the returned frames',
                 gpu_share_of_host=found['enlarge_on_the_gpu_ms']['median'] / found['full_size_then_pillow_ms']['median'])
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--video-frames', type=int, default=75)
    ap.add_argument('--calls', type=int, default=3, help='per arm of the route, after one warm-up')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'enlarge.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('enlarge_time.py measures on a GPU, and there is none')
    widths = (1920 * args.size // 1024, 4 * int(0.9 * args.size))
    line = dict(what='the bicubic enlargement: the entry alone, the crop of 0.9 of the side to 1920 wide and 4-fold, each beside a device-to-device copy of as much traffic, and the bilinear '
                     'enlargement of the same crop to the photo\'s size; and a delivered video enlarged on the GPU against the same at full size enlarged by Pillow on the host',
                size=args.size, gpu=torch.cuda.get_device_name(0), kernel=kernel_times(args.size, args.frames, widths), route=route_times(args.size, args.video_frames, args.calls, widths[0]))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
