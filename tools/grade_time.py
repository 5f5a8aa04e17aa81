#!/usr/bin/env python3
"""What a colour grade costs (grade.py), arms taking turns in this one process:
  kernel:  HIP events around the grade's entry alone -- the raw entry on frames and a table that lie in HBM already, nothing allocated --,
           FRAMES frames of SIZE x SIZE per call, in place, at strength 256: a table of 17 nodes per axis and one of 33, both of noise.  A
           sample is LAUNCHES = 20 calls back to back between two events, divided by 20; three turns of warm-up and then the median of 10
           samples each.  The grade reads 3 bytes per pixel and writes 3: its traffic is 6 bytes per pixel and frame (the table's copies
           into LDS come on top and are not counted), and its rate is that traffic over its time.  In the same turns a device-to-device
           copy_ of as many bytes (it reads half of them and writes half), and overlay.py's full-frame overlay on the same frames, the
           nearest in-place kernel there is, which moves 10 bytes per pixel.  Reported: every arm's median, minimum and maximum, the grades'
           rates, their shares of the copy's rate and of the overlay's rate, N = 33's time over N = 17's, and what the table's copies are per
           launch: the workgroups of the launch times the table's bytes.
  route:   wall clock, one synthetic photo of SIZE with seeded weights, one Pipeline: a delivered video of VIDEO_FRAMES frames with
           look='sepia' against the same video without a grade, both writing their video.
One JSON line on stdout and in --out (default profiles/grade.json).  Needs a GPU: without one it exits with an error."""
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
SIZES = (17, 33)
# csrc/kbe_grade.hip: the workgroups a launch has at most (256 CUs x those a CU holds at the table's LDS size) and the waves of one, each
# with 1024 pixels of a row per trip
MOST_GROUPS = {17: (256 * 8, 4), 33: (256 * 1, 16)}


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
    from ken_burns_effect_amd import _native, grade, overlay
    a = torch.randint(0, 256, (frames, size, size, 3), dtype=torch.uint8, device='cuda')
    tables = {N: torch.randint(0, 256, (N, N, N, 4), dtype=torch.uint8, device='cuda') for N in SIZES}
    picture = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device='cuda')
    traffic = {'grade': 6 * size * size * frames, 'overlay': 10 * size * size * frames}
    source, target = torch.randint(0, 256, (traffic['grade'] // 2,), dtype=torch.uint8, device='cuda'), torch.empty(traffic['grade'] // 2, dtype=torch.uint8, device='cuda')
    table = pointers(a)
    full = (ctypes.c_int32 * frames)(*[256] * frames)
    zeros = (ctypes.c_int32 * frames)(*[0] * frames)

    def grade_arm(N):
        lut = tables[N]
        return lambda: grade._call('kbe_grade_u8', table, frames, size, size, 3 * size, lut.data_ptr(), N, full, _native._stream())
    arms = {'grade_%d' % N: grade_arm(N) for N in SIZES}
    arms['overlay_full'] = lambda: overlay._call('kbe_overlay_u8', table, frames, size, size, 3 * size, picture.data_ptr(), size, size, 4 * size, zeros, zeros, full, _native._stream())
    arms['copy'] = lambda: target.copy_(source)
    # the arm is the entry grade.apply calls: one frame through both, the same bytes
    check = a[:1].clone()
    want = grade.apply(check.clone(), tables[33])
    grade._call('kbe_grade_u8', pointers(check), 1, size, size, 3 * size, tables[33].data_ptr(), 33, (ctypes.c_int32 * 1)(256), _native._stream())
    assert torch.equal(check, want) and not torch.equal(want, a[:1])
    ms = {name: [] for name in arms}
    for turn in range(13):                                        # three turns of warm-up, then ten, the arms taking turns
        for name, arm in arms.items():
            t = timed(arm)
            if turn >= 3:
                ms[name].append(t)
    found = {name + '_ms': stats(t) for name, t in ms.items()}
    rate = {name: traffic['overlay' if name == 'overlay_full' else 'grade'] / (1e6 * found[name + '_ms']['median']) for name in arms}      # bytes / (1e-3 s) / 1e9
    found.update(frames=frames, launches_per_sample=LAUNCHES, traffic_bytes_per_call=traffic, GB_per_s=rate,
                 share_of_the_copys_rate={name: rate[name] / rate['copy'] for name in arms if name != 'copy'},
                 grade_share_of_the_overlays_rate={'grade_%d' % N: rate['grade_%d' % N] / rate['overlay_full'] for N in SIZES},
                 grade_33_time_over_grade_17=found['grade_33_ms']['median'] / found['grade_17_ms']['median'])
    copies = {}
    for N in SIZES:
        most, waves = MOST_GROUPS[N]
        items = frames * size * ((size + 1023) // 1024)
        groups = min((items + waves - 1) // waves, most)
        copies['grade_%d' % N] = {'workgroups': groups, 'table_bytes': 4 * N ** 3, 'bytes_per_launch': groups * 4 * N ** 3,
                                  'share_of_the_frames_traffic': groups * 4 * N ** 3 / traffic['grade']}
    found['table_copies_per_launch'] = copies
    return found


def route_times(size, frames, calls):
    from ken_burns_effect_amd import kbe, slideshow, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    image = synthetic.make_rgbd(size, size, 0)[0]
    zoom = kbe.windows_for(size, size, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, device='cuda:0', steps=frames, miopen_find=False)
    with tempfile.TemporaryDirectory() as tmp:
        def deliver(look):
            pipe.look = look
            pipe(image, zoom, os.path.join(tmp, look or 'plain'))
        arms = {'plain': lambda: deliver(None), 'sepia': lambda: deliver('sepia')}
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
    found.update(photo_size=size, frames=frames, jpeg=os.environ.get('KBE_JPEG', 'native'), sepia_share_of_plain=found['sepia_ms']['median'] / found['plain_ms']['median'])
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--video-frames', type=int, default=75)
    ap.add_argument('--calls', type=int, default=3, help='per arm of the route, after one warm-up')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grade.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('grade_time.py measures on a GPU, and there is none')
    line = dict(what='colour grading: the entry alone with tables of 17 and of 33 nodes per axis, beside a device-to-device copy of as much traffic and the full-frame overlay on the same '
                     'frames, and a delivered video with look=sepia against the same without',
                size=args.size, gpu=torch.cuda.get_device_name(0), kernel=kernel_times(args.size, args.frames), route=route_times(args.size, args.video_frames, args.calls))
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
