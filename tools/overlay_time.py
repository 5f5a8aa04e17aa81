#!/usr/bin/env python3
"""What an overlay costs (overlay.py), arms taking turns in this one process:
  kernel:  HIP events around the overlay's entry alone -- the raw entry on frames and a picture that lie in HBM already, nothing allocated --,
           FRAMES frames of SIZE x SIZE per call, in place: a full-frame overlay (SIZE x SIZE at 0,0) and a caption-sized rectangle (640 x 64
           near the bottom), both of noise with every alpha, at opacity 256.  A sample is LAUNCHES = 20 calls back to back between two
           events, divided by 20; three turns of warm-up and then the median of 10 samples each.  The overlay reads 3 frame bytes and 4
           overlay bytes per pixel of its rectangle and writes 3: its traffic is 10 bytes per pixel and frame, and its rate is that traffic
           over its time.  In the same turns, for each of the two, a device-to-device copy_ whose traffic is as many bytes (it reads half of
           them and writes half), and transition.py's dissolve on the same frames, which moves 9 bytes per pixel -- the yardstick, no fixed
           number: 10 / 9 = 1.11 of the dissolve's time is the traffic alone.  Reported: every arm's median, minimum and maximum, the
           overlays' rates, their shares of their copies' rates, and the full-frame overlay's time as a share of the dissolve's.
  route:   wall clock, one synthetic photo of SIZE with seeded weights, one Pipeline: a delivered video of VIDEO_FRAMES frames with a
           watermark of 200 x 60 against the same video without one, both writing their video.
One JSON line on stdout and in --out (default profiles/overlay.json).  Needs a GPU: without one it exits with an error."""
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


LAUNCHES = 20          # back-to-back calls between the two events of one sample: a single call of 30 us is too close to the events' own resolution
CAPTION = (640, 64)


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


def kernel_times(size, frames):
    from ken_burns_effect_amd import _native, overlay, transition
    a = torch.randint(0, 256, (frames, size, size, 3), dtype=torch.uint8, device='cuda')
    b = torch.randint(0, 256, (frames, size, size, 3), dtype=torch.uint8, device='cuda')
    out = torch.empty(frames, size, size, 3, dtype=torch.uint8, device='cuda')
    w, h = min(CAPTION[0], size), min(CAPTION[1], size)
    pictures = {'full': torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device='cuda'), 'caption': torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device='cuda')}
    places = {'full': (0, 0), 'caption': ((size - w) // 2, size - h - size // 32)}
    traffic = {name: 10 * p.shape[0] * p.shape[1] * frames for name, p in pictures.items()}
    copies = {name: (torch.randint(0, 256, (t // 2,), dtype=torch.uint8, device='cuda'), torch.empty(t // 2, dtype=torch.uint8, device='cuda')) for name, t in traffic.items()}
    tables = pointers(a), pointers(b), pointers(out)
    opaque = (ctypes.c_int32 * frames)(*[256] * frames)

    def overlay_arm(name):
        picture = pictures[name]
        xs, ys = ((ctypes.c_int32 * frames)(*[v] * frames) for v in places[name])
        return lambda: overlay._call('kbe_overlay_u8', tables[0], frames, size, size, 3 * size, picture.data_ptr(), picture.shape[1], picture.shape[0], 4 * picture.shape[1], xs, ys, opaque,
                                     _native._stream())
    check = a[:1].clone()
    want = overlay.apply(check.clone(), pictures['caption'], places['caption'][0], places['caption'][1])
    arms = {name: overlay_arm(name) for name in pictures}
    half = (ctypes.c_int32 * frames)(*[128] * frames)
    arms['dissolve'] = lambda: transition._call('kbe_transition_u8', tables[0], tables[1], frames, size, size, 3 * size, transition.KINDS['dissolve'], half, 1, 0, tables[2], 3 * size,
                                                _native._stream())
    for name, (source, target) in copies.items():
        arms['copy_' + name] = lambda source=source, target=target: target.copy_(source)
    a[:1].copy_(check)
    arms['caption']()
    assert torch.equal(a[:1], want) and not torch.equal(want, check)
    ms = {name: [] for name in arms}
    for turn in range(13):                                        # three turns of warm-up, then ten, the arms taking turns
        for name, arm in arms.items():
            t = timed(arm)
            if turn >= 3:
                ms[name].append(t)
    found = {name + '_ms': stats(t) for name, t in ms.items()}
    rate = {name: traffic[name.replace('copy_', '')] / (1e6 * found[name + '_ms']['median']) for name in ('full', 'caption', 'copy_full', 'copy_caption')}      # bytes / (1e-3 s) / 1e9
    found.update(frames=frames, launches_per_sample=LAUNCHES, caption=list(CAPTION), traffic_bytes_per_call=traffic, full_GB_per_s=rate['full'], caption_GB_per_s=rate['caption'],
                 copy_full_GB_per_s=rate['copy_full'], copy_caption_GB_per_s=rate['copy_caption'], full_share_of_its_copys_rate=rate['full'] / rate['copy_full'],
                 caption_share_of_its_copys_rate=rate['caption'] / rate['copy_caption'], full_time_as_a_share_of_the_dissolves=found['full_ms']['median'] / found['dissolve_ms']['median'],
                 the_traffic_alone_as_a_share_of_the_dissolves=10.0 / 9.0)
    return found


def route_times(size, frames, calls):
    from PIL import Image
    from ken_burns_effect_amd import kbe, slideshow, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    image = synthetic.make_rgbd(size, size, 0)[0]
    zoom = kbe.windows_for(size, size, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, device='cuda:0', steps=frames, miopen_find=False)
    with tempfile.TemporaryDirectory() as tmp:
        logo = np.random.default_rng(0).integers(0, 256, (60, 200, 4), dtype=np.uint8)
        Image.fromarray(logo, 'RGBA').save(os.path.join(tmp, 'logo.png'))

        def deliver(watermark):
            pipe.overlay = os.path.join(tmp, 'logo.png') if watermark else None
            pipe(image, zoom, os.path.join(tmp, 'watermark' if watermark else 'plain'))
        arms = {'plain': lambda: deliver(False), 'watermark': lambda: deliver(True)}
        times = {name: [] for name in arms}
        for turn in range(calls + 1):                             # one turn of warm-up
            for name, arm in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm()
                torch.cuda.synchronize()
                if turn >= 1:
                    times[name].append(1e3 * (time.perf_counter() - t0))
    found = {name + '_ms': stats(t) for name, t in times.items()}
    found.update(photo_size=size, frames=frames, watermark=[200, 60], jpeg=os.environ.get('KBE_JPEG', 'native'),
                 watermark_share_of_plain=found['watermark_ms']['median'] / found['plain_ms']['median'])
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--video-frames', type=int, default=75)
    ap.add_argument('--calls', type=int, default=3, help='per arm of the route, after one warm-up')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'overlay.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('overlay_time.py measures on a GPU, and there is none')
    line = dict(what='overlays: the entry alone, a full-frame overlay and a caption-sized one, beside device-to-device copies of as much traffic and the dissolve on the same frames, '
                     'and a delivered video with a watermark against the same without',
                size=args.size, gpu=torch.cuda.get_device_name(0), kernel=kernel_times(args.size, args.frames), route=route_times(args.size, args.video_frames, args.calls))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
