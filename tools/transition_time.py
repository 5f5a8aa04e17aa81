#!/usr/bin/env python3
"""What a transition costs (transition.py, slideshow.py), arms taking turns in this one process:
  kernel:  HIP events around kbe_transition_u8 alone -- the raw entry on frames and outputs that lie in HBM already, nothing allocated --,
           OUTPUTS frames of SIZE x SIZE per call, one arm per kind: the dissolve at p = 128, the four wipes at p = 128 with s = an eighth of
           their extent, the fade at p = 64.  A sample is LAUNCHES = 20 calls back to back between two events, divided by 20; three turns of warm-up
           and then the median of 10 samples each.  The dissolve reads two frames and writes one:
           its traffic is 3 * 3 W H bytes per output, and its rate is that traffic over its time.  In the same turns a device-to-device
           copy_ whose traffic is as many bytes (it reads half of them and writes half) -- the yardstick, no fixed number -- and
           kbe_shutter_mean_u8 at S = 2, which moves the bytes the dissolve moves.  Reported: every arm's median, minimum and maximum, the
           dissolve's median against the shutter arm's median plus that arm's own spread (max - min), the dissolve's share of the copy's
           rate, and every wipe's time as a share of the dissolve's (a wipe does not read the source it does not need outside its edge).
  route:   wall clock, on PHOTOS synthetic photos of PHOTO_SIZE with seeded weights, one Pipeline: slideshow.make of the photos (clips of
           FRAMES steps, T = 12, a dissolve) against the same photos delivered separately, one Pipeline call each, both writing their video.
One JSON line on stdout and in --out (default profiles/transition.json).  Needs a GPU: without one it exits with an error."""
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


def kernel_times(size, outputs):
    from ken_burns_effect_amd import _native, shutter, transition
    a = torch.randint(0, 256, (outputs, size, size, 3), dtype=torch.uint8, device='cuda')
    b = torch.randint(0, 256, (outputs, size, size, 3), dtype=torch.uint8, device='cuda')
    out = torch.empty(outputs, size, size, 3, dtype=torch.uint8, device='cuda')
    pairs = torch.stack([a, b], dim=1).reshape(2 * outputs, size, size, 3).contiguous()       # the shutter's sources: (a[i], b[i]) for output i
    traffic = 3 * 3 * size * size * outputs
    source, target = torch.randint(0, 256, (traffic // 2,), dtype=torch.uint8, device='cuda'), torch.empty(traffic // 2, dtype=torch.uint8, device='cuda')
    tables = pointers(a), pointers(b), pointers(out), pointers(pairs)

    def kind_arm(kind, p):
        progress = (ctypes.c_int32 * outputs)(*[p] * outputs)
        softness = transition.default_softness(kind, size, size)
        return lambda: transition._call('kbe_transition_u8', tables[0], tables[1], outputs, size, size, 3 * size, transition.KINDS[kind], progress, softness, 0,
                                        tables[2], 3 * size, _native._stream())
    arms = {kind: kind_arm(kind, 64 if kind == 'fade' else 128) for kind in transition.KINDS}
    arms['shutter_S2'] = lambda: shutter._call('kbe_shutter_mean_u8', tables[3], outputs, 2, size, size, 3 * size, tables[2], 3 * size, _native._stream())
    arms['copy'] = lambda: target.copy_(source)
    ms = {name: [] for name in arms}
    for turn in range(13):                                        # three turns of warm-up, then ten, the arms taking turns
        for name, arm in arms.items():
            t = timed(arm)
            if turn >= 3:
                ms[name].append(t)
    arms['dissolve']()
    assert torch.equal(out[:1], transition.blend(a[:1], b[:1], 'dissolve', [128]))
    found = {name + '_ms': stats(t) for name, t in ms.items()}
    dissolve, reference = found['dissolve_ms'], found['shutter_S2_ms']
    rate = {name: traffic / (1e6 * found[name + '_ms']['median']) for name in ('dissolve', 'shutter_S2', 'copy')}           # bytes / (1e-3 s) / 1e9
    found.update(outputs=outputs, launches_per_sample=LAUNCHES, traffic_bytes_per_call=traffic, dissolve_GB_per_s=rate['dissolve'], shutter_S2_GB_per_s=rate['shutter_S2'], copy_GB_per_s=rate['copy'],
                 dissolve_share_of_the_copys_rate=rate['dissolve'] / rate['copy'], shutter_S2_spread_ms=reference['max'] - reference['min'],
                 dissolve_within_the_shutters_median_plus_spread=dissolve['median'] <= reference['median'] + (reference['max'] - reference['min']),
                 time_as_a_share_of_the_dissolves={kind: found[kind + '_ms']['median'] / dissolve['median'] for kind in transition.KINDS})
    return found


def route_times(size, photos, frames, calls):
    from ken_burns_effect_amd import kbe, slideshow, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    images = [synthetic.make_rgbd(size, size, seed)[0] for seed in range(photos)]
    zoom = kbe.windows_for(size, size, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, device='cuda:0', steps=frames, miopen_find=False)
    with tempfile.TemporaryDirectory() as tmp:
        arms = {'slideshow': lambda: slideshow.make(images, os.path.join(tmp, 'show'), pipe, 'dissolve', 12),
                'separate': lambda: [pipe(image, zoom, os.path.join(tmp, 'clip%d' % k)) for k, image in enumerate(images)]}
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
    found.update(photos=photos, photo_size=size, frames_per_clip=frames, transition_frames=12, slideshow_frames=photos * frames - (photos - 1) * 12, separate_frames=photos * frames,
                 jpeg=os.environ.get('KBE_JPEG', 'native'), slideshow_share_of_separate=found['slideshow_ms']['median'] / found['separate_ms']['median'])
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--outputs', type=int, default=12)
    ap.add_argument('--photos', type=int, default=3)
    ap.add_argument('--photo-size', type=int, default=512)
    ap.add_argument('--frames', type=int, default=75)
    ap.add_argument('--calls', type=int, default=3, help='per arm of the route, after one warm-up')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transition.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('transition_time.py measures on a GPU, and there is none')
    line = dict(what='transitions: kbe_transition_u8 alone per kind beside a device-to-device copy of as much traffic and kbe_shutter_mean_u8 at S = 2, '
                     'and a slideshow against its photos delivered separately',
                size=args.size, gpu=torch.cuda.get_device_name(0), kernel=kernel_times(args.size, args.outputs),
                route=route_times(args.photo_size, args.photos, args.frames, args.calls))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
