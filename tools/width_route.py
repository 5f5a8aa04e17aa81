#!/usr/bin/env python3
"""A delivered video at a chosen width (common.render_frames(out_size=...), crop_area.py) beside the video at the photo's size, on the bench's
scene (bench.build_scene, inpainted cloud), SIZE x SIZE frames reduced to WIDTH wide:
  reduce:  crop_area.reduce alone on FRAMES raw frames that lie in HBM, HIP events around the call (its output's allocation included);
  arms, taking turns in this one process, wall clock around calls that end with the frames in host memory:
    full      render_frames(cameras, oc, crop): today's frames, fetched at full size;
    reduced   render_frames(cameras, oc, crop, out_size=(w, h)): rendered raw into HBM, crop + area average there, fetched reduced;
    full_then_pillow   the only way to a narrower video before out_size: `full`, then Pillow's resize((w, h), Image.BOX) of every frame on
              the host, one thread (another filter and two resamplings: tests/test_crop_area_stream.py has the quality of the two routes).
One JSON line on stdout and, with --out, in a file.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from ken_burns_effect_amd import common, crop_area, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=75)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--seconds', type=float, default=3.0, help='per arm, and at least three calls')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'width_route.py measures on a GPU'
    from PIL import Image
    size, n = args.size, args.frames
    ofrom, oto = synthetic.default_windows(size, size, False)
    settings = {'dblSteps': [i / (n - 1) for i in range(n)], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False}
    oc = bench.build_scene(size, torch.device('cuda:0'), True, dict(settings, boolInpaint=True))
    cameras, crop = common.frame_cameras(settings, oc), common.crop_size(settings)
    out_size = crop_area.size_for(size, size, width=args.width)

    def full():
        return common.render_frames(cameras, oc, crop)

    def reduced():
        return common.render_frames(cameras, oc, crop, out_size=out_size)

    def full_then_pillow():
        return [np.asarray(Image.fromarray(frame).resize(out_size, Image.BOX)) for frame in full()]

    arms = {'full': full, 'reduced': reduced, 'full_then_pillow': full_then_pillow}
    shapes = {name: tuple(np.shape(arm())) for name, arm in arms.items()}           # warm-up, and what comes back
    assert shapes['full'] == (n, size, size, 3) and shapes['reduced'] == shapes['full_then_pillow'] == (n, out_size[1], out_size[0], 3), shapes
    times = {name: [] for name in arms}
    while True:                                                       # taking turns; an arm stops once it has its SECONDS and three calls (Pillow's takes 0.2 s a call)
        wanted = [(name, arm) for name, arm in arms.items() if sum(times[name]) < args.seconds or len(times[name]) < 3]
        if not wanted:
            break
        for name, arm in wanted:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    raw = common.render_frames(cameras, oc, None, keep_on_device=True)
    reduce_ms = []
    for _ in range(11):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        crop_area.reduce(raw, crop, out_size)
        e1.record()
        torch.cuda.synchronize()
        reduce_ms.append(e0.elapsed_time(e1))
    reduce_ms = reduce_ms[1:]
    line = dict(what='a delivered video at a chosen width beside the video at the photo\'s size', size=size, frames=n, crop=list(crop), out_size=list(out_size),
                gpu=torch.cuda.get_device_name(0), points=int(oc['tensorInpaPoints'].shape[2]),
                crop_area_reduce_ms_per_video={'median': float(np.median(reduce_ms)), 'min': min(reduce_ms), 'max': max(reduce_ms), 'calls': len(reduce_ms), 'with_its_allocation': True},
                crop_area_reduce_us_per_frame=1e3 * float(np.median(reduce_ms)) / n,
                bytes_fetched={'full': n * size * size * 3, 'reduced': n * out_size[0] * out_size[1] * 3},
                **{name + '_ms_per_video': {'median': 1e3 * float(np.median(t)), 'min': 1e3 * min(t), 'max': 1e3 * max(t), 'calls': len(t)} for name, t in times.items()})
    line['reduced_over_full'] = line['reduced_ms_per_video']['median'] / line['full_ms_per_video']['median']
    line['full_then_pillow_over_reduced'] = line['full_then_pillow_ms_per_video']['median'] / line['reduced_ms_per_video']['median']
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
