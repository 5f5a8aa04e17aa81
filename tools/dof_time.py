#!/usr/bin/env python3
"""What depth of field costs (dof.py, common.render_frames(lens=...)), on the bench's scene (bench.build_scene, inpainted cloud), SIZE x SIZE frames:
  k_dof:   dof.apply alone on ONE raw frame that lies in HBM with the depth plane its float render holds, the focus at the median depth, HIP
           events around the call (its output's allocation included), medians: at aperture 0 (the copy floor) and at the apertures and caps
           that put a tenth of this frame's pixels at radius 4, 8 and 16 (and the rest below);
  arms, taking turns in this one process, wall clock around calls that end with the FRAMES frames in host memory:
    plain       render_frames(cameras, oc, crop): the video without a lens, the route it takes today (kbe_render_video);
    lens_still  render_frames(cameras, oc, crop, lens=...) with an aperture of 1e-6: every radius 0, the gather a copy -- what the lens
                route's per-frame render_frame, float renders and crop_resize cost beside `plain`;
    lens_4, lens_8, lens_16   the same route at the three apertures, the focus pulled from the 30th to the 70th percentile of the depths.
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
from ken_burns_effect_amd import common, dof, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=75)
    ap.add_argument('--seconds', type=float, default=2.0, help='per arm, and at least three calls')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'dof_time.py measures on a GPU'
    size, n = args.size, args.frames
    ofrom, oto = synthetic.default_windows(size, size, False)
    settings = {'dblSteps': [i / (n - 1) for i in range(n)], 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False}
    oc = bench.build_scene(size, torch.device('cuda:0'), True, dict(settings, boolInpaint=True))
    cameras, crop = common.frame_cameras(settings, oc), common.crop_size(settings)
    K = common._K()
    state = common._prepared_cloud(K, oc)

    # one frame in the middle of the path, and its depths
    focal, shift3 = cameras[n // 2]
    render = torch.zeros(1, 4, size, size, device='cuda')
    raw = K.render_frame(state, shift3, focal, oc['dblBaseline'], render_f32=render[0]).clone()[None]
    z = render[0, 3].cpu().numpy().astype(np.float64)
    good = np.isfinite(z) & (z > 0)
    focus = float(np.median(z[good]))
    spread = float(np.percentile(np.abs(z[good] - focus) / z[good], 90))    # the 90th percentile of |z - zf| / z: at an aperture of r / spread and the cap r a tenth of the pixels sit at radius r
    apertures = {'0': 0.0, '4': 4.0 / spread, '8': 8.0 / spread, '16': 16.0 / spread}
    caps = {'0': 16, '4': 4, '8': 8, '16': 16}
    kernel = {}
    for name, aperture in apertures.items():
        ms = []
        for _ in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = dof.apply(raw, render[:, 3], [focus], aperture, caps[name])
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = ms[2:]
        zf, a = np.float32(focus), np.float32(aperture)
        r = np.zeros(z.shape, np.int64)
        with np.errstate(all='ignore'):
            lhs = a * np.abs(z.astype(np.float32) - zf)
            for j in range(1, caps[name] + 1):
                r += lhs >= np.float32(j - 0.5) * z.astype(np.float32)
        r[~good] = 0
        kernel['radius_' + name] = {'aperture': aperture, 'max_radius': caps[name], 'ms_per_frame': {'median': float(np.median(ms)), 'min': min(ms), 'max': max(ms), 'calls': len(ms), 'with_its_allocation': True},
                                    'largest_radius': int(r.max()), 'mean_radius': float(r.mean()), 'pixels_blurred': float((r > 0).mean()),
                                    'bytes_changed': float((out != raw).float().mean().item())}

    near, far = float(np.percentile(z[good], 30)), float(np.percentile(z[good], 70))
    arms = {'plain': lambda: common.render_frames(cameras, oc, crop),
            'lens_still': lambda: common.render_frames(cameras, oc, crop, lens=dof.Lens(near, far, 1e-6)),
            'lens_4': lambda: common.render_frames(cameras, oc, crop, lens=dof.Lens(near, far, apertures['4'], 4)),
            'lens_8': lambda: common.render_frames(cameras, oc, crop, lens=dof.Lens(near, far, apertures['8'], 8)),
            'lens_16': lambda: common.render_frames(cameras, oc, crop, lens=dof.Lens(near, far, apertures['16'], 16))}
    shapes = {name: tuple(np.shape(arm())) for name, arm in arms.items()}           # warm-up, and what comes back
    assert all(shape == (n, size, size, 3) for shape in shapes.values()), shapes
    times = {name: [] for name in arms}
    while True:                                                       # taking turns; an arm stops once it has its SECONDS and three calls
        wanted = [(name, arm) for name, arm in arms.items() if sum(times[name]) < args.seconds or len(times[name]) < 3]
        if not wanted:
            break
        for name, arm in wanted:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    line = dict(what='depth of field: the gather alone on one frame, and a delivered video with and without a lens', size=size, frames=n, crop=list(crop),
                gpu=torch.cuda.get_device_name(0), points=int(oc['tensorInpaPoints'].shape[2]), focus=focus, spread=spread, focus_pull=[near, far], k_dof=kernel,
                **{name + '_ms_per_video': {'median': 1e3 * float(np.median(t)), 'min': 1e3 * min(t), 'max': 1e3 * max(t), 'calls': len(t)} for name, t in times.items()})
    line['lens_still_over_plain'] = line['lens_still_ms_per_video']['median'] / line['plain_ms_per_video']['median']
    line['gather_ms_per_frame_in_the_route'] = {r: (line['lens_%s_ms_per_video' % r]['median'] - line['lens_still_ms_per_video']['median']) / n for r in ('4', '8', '16')}
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
