#!/usr/bin/env python3
"""Frames that lie in HBM -> the PNG files of --write-frames in host memory, two ways in the SAME run, taking turns:
  device: HipKernels.png_encode (kbe_png_encode: the GPU encodes, the files cross the link);
  host:   the frames cross the link raw into pinned memory and pipeline.png_bytes encodes them on the writers' host threads (zlib level 1).
Wall clock around calls that end with the bytes on the host (the device's ends in a device synchronise), every arm warmed up, SECONDS per
arm and size.  One JSON line per size on stdout and, with --out, in a file.  --profile: nothing but ROUNDS device encodes of each size
(for a `rocprofv3 --kernel-trace --stats` run of its own).  Needs a GPU."""
import argparse
import ctypes
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ken_burns_effect_amd import _native, pipeline  # noqa: E402


def photo_like(n, size, device):
    """n distinct frames with the statistics of tests/test_jpeg_writer.py's photo_like (smooth colour, an edge, sensor noise), made on the GPU."""
    g = torch.Generator(device=device).manual_seed(7)
    yy, xx = torch.meshgrid(torch.arange(size, device=device, dtype=torch.float32), torch.arange(size, device=device, dtype=torch.float32), indexing='ij')
    frames = torch.empty(n, size, size, 3, dtype=torch.uint8, device=device)
    for i in range(n):
        img = torch.stack([128 + 100 * torch.sin(xx / 23.0 + 0.05 * i) * torch.cos(yy / 31.0), 128 + 90 * torch.sin((xx + yy + 3 * i) / 41.0), 255.0 * xx / (size - 1)], -1)
        img[size // 4:size // 2, size // 3 + i:2 * size // 3 + i] = torch.tensor([220.0, 40.0, 60.0], device=device)
        frames[i] = (img + 4 * torch.randn(img.shape, generator=g, device=device)).clamp(0, 255).to(torch.uint8)
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='512x64,1024x75', help='SIZExFRAMES, comma separated')
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--threads', type=int, default=16, help='host threads of the host arm')
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'png_time.py measures on a GPU'
    K = _native.kernels()
    pipeline.WRITER_THREADS = args.threads
    os.environ.pop('KBE_WRITER_THREADS', None)
    lines = []
    for spec in args.sizes.split(','):
        size, n = (int(v) for v in spec.split('x'))
        frames = photo_like(n, size, torch.device('cuda'))
        pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()

        def device_arm():
            return K.png_encode(frames)

        def host_arm():
            pinned.copy_(frames, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = pinned.numpy()
            return pipeline._on_threads([host[i] for i in range(n)], pipeline.png_bytes)

        if args.profile:
            for _ in range(args.rounds):
                device_arm()
            torch.cuda.synchronize()
            continue
        on_device, on_host = device_arm(), host_arm()                   # warm-up, and the files to look at
        device_arm(), host_arm()
        times = {'device': [], 'host': []}
        while min(sum(times['device']), sum(times['host'])) < args.seconds:
            for name, arm in (('device', device_arm), ('host', host_arm)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        # the device alone: the launches of a call on buffers that exist, HIP events
        lib = K.lib
        scratch = torch.empty(int(lib.kbe_png_scratch_bytes(size, size, n)) // 8 + 1, dtype=torch.int64, device='cuda')
        cap = sum(len(s) for s in on_device)
        files = torch.empty(cap, dtype=torch.uint8, device='cuda')
        meta = torch.empty(n + 2, dtype=torch.int64, device='cuda')
        pointers = (ctypes.c_void_p * n)(*[frames.data_ptr() + i * size * size * 3 for i in range(n)])
        kernel_ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = lib.kbe_png_encode(pointers, n, size, size, 3 * size, 0, ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(files.data_ptr()), ctypes.c_size_t(cap),
                                    ctypes.c_void_p(meta.data_ptr()), ctypes.c_void_p(meta.data_ptr() + 8 * (n + 1)), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0
            kernel_ms.append(e0.elapsed_time(e1))
        # lossless: the first and the last file decode to their frames
        from PIL import Image
        for i in (0, n - 1):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(on_device[i])).convert('RGB')), frames[i].cpu().numpy())
        line = {'what': 'frames in HBM -> PNG files on the host', 'size': size, 'frames': n, 'host_threads': args.threads,
                'device_ms_per_video': {'median': 1e3 * float(np.median(times['device'])), 'min': 1e3 * min(times['device']), 'max': 1e3 * max(times['device']), 'calls': len(times['device'])},
                'host_ms_per_video': {'median': 1e3 * float(np.median(times['host'])), 'min': 1e3 * min(times['host']), 'max': 1e3 * max(times['host']), 'calls': len(times['host'])},
                'device_over_host_speedup': float(np.median(times['host']) / np.median(times['device'])),
                'device_kernels_only_ms_per_video': {'median': float(np.median(kernel_ms)), 'min': min(kernel_ms)},
                'device_file_bytes': cap, 'host_file_bytes': sum(len(s) for s in on_host), 'raw_bytes': n * size * size * 3,
                'device_over_host_bytes': cap / sum(len(s) for s in on_host), 'gpu': torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
