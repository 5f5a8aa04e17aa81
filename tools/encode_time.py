#!/usr/bin/env python3
"""Frames that lie in HBM -> Motion-JPEG streams (--format mjpeg), the PNG files of --write-frames (--format png) or an animated GIF (--format
gif) in host memory, two ways in the SAME run, taking turns:
  device: HipKernels.mjpeg_encode / png_encode (kbe_mjpeg_encode, kbe_png_encode: the GPU encodes, the streams or files cross the link);
          gif: what gif.write_gif does short of the file -- histogram, palette (host), table, kbe_gif_encode, assemble;
  host:   the frames cross the link raw into pinned memory and the writers' host threads encode them (mjpeg: libkbe_jpeg.so,
          kbe_jpeg_encode_batch; png: pipeline.png_bytes, zlib level 1; gif: Pillow's save(format='GIF', save_all=True), one thread).
Wall clock around calls that end with the bytes on the host (the device's ends in a device synchronise), every arm warmed up, SECONDS per
arm and size.  With --gif-width and/or --gif-every (--format gif), instead: the device route at the frames' own size and every frame (as above)
against the same route at that width (area.reduce, the exact area average on the GPU, the height by area.size_for) and every so-many-th frame,
both short of the file, and the bytes of the files they would write, forth and back.  One JSON line per size on stdout and, with --out, in a file.  --profile: nothing but ROUNDS device encodes of each size
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

from ken_burns_effect_amd import _native, area, gif, pipeline  # noqa: E402


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


def gif_reduced_main(args):
    """--format gif --gif-width N / --gif-every K: what gif.write_gif does short of the file, at the frames' own size and every frame against
    size=(N, its height), every=K; milliseconds per clip, the bytes of the file (forth and back), and area.reduce alone by HIP events."""
    lines = []
    for spec in args.sizes.split(','):
        size, n = (int(v) for v in spec.split('x'))
        frames = photo_like(n, size, torch.device('cuda'))
        w, h = area.size_for(size, size, width=args.gif_width)
        kept = gif.kept_frames(n, args.gif_every)
        index = torch.tensor(kept, device=frames.device)

        def route(reduced):
            chosen = frames
            if reduced:
                chosen = frames.index_select(0, index) if args.gif_every != 1 else frames
                chosen = area.reduce(chosen, w, h) if (w, h) != (size, size) else chosen
            palette = gif.palette_from_histogram(gif.histogram(chosen))
            units = gif.encode(chosen, gif.lut(palette), dither='ordered', delay_cs=gif.delay_for(25.0 / (args.gif_every if reduced else 1)))
            return gif.assemble(units + units[-2::-1], int(chosen.shape[2]), int(chosen.shape[1]), palette)

        files = {'full': route(False), 'reduced': route(True)}           # warm-up, and the bytes to look at
        if args.profile:
            for _ in range(args.rounds):
                route(True)
            torch.cuda.synchronize()
            continue
        times = {'full': [], 'reduced': []}
        while any(sum(t) < args.seconds or len(t) < 3 for t in times.values()):          # taking turns
            for name in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                route(name == 'reduced')
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        chosen = frames.index_select(0, index)
        reduce_ms = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            area.reduce(chosen, w, h)
            e1.record()
            torch.cuda.synchronize()
            reduce_ms.append(e0.elapsed_time(e1))
        line = dict(what='frames in HBM -> an animated GIF on the host, at their own size and reduced', size=size, frames=n, gpu=torch.cuda.get_device_name(0),
                    gif_size=[w, h], gif_every=args.gif_every, frames_kept=len(kept),
                    full_ms_per_clip=1e3 * float(np.median(times['full'])), reduced_ms_per_clip=1e3 * float(np.median(times['reduced'])),
                    full_file_bytes=len(files['full']), reduced_file_bytes=len(files['reduced']), calls={name: len(t) for name, t in times.items()},
                    area_reduce_ms_per_clip={'median': float(np.median(reduce_ms)), 'min': min(reduce_ms), 'with_its_allocation': True})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


def gif_main(args):
    """--format gif: the device route (the whole of it, and its stages one by one with HIP events and a host clock) against raw delivery +
    Pillow; microseconds and bytes per frame."""
    from PIL import Image
    lines = []
    for spec in args.sizes.split(','):
        size, n = (int(v) for v in spec.split('x'))
        frames = photo_like(n, size, torch.device('cuda'))
        pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()

        def device_arm():
            palette = gif.palette_from_histogram(gif.histogram(frames))
            return gif.assemble(gif.encode(frames, gif.lut(palette), dither='ordered'), size, size, palette)

        def host_arm():
            pinned.copy_(frames, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = pinned.numpy()
            images = [Image.fromarray(host[i]) for i in range(n)]
            out = io.BytesIO()
            images[0].save(out, format='GIF', save_all=True, append_images=images[1:], duration=40, loop=0)
            return out.getvalue()

        if args.profile:
            for _ in range(args.rounds):
                device_arm()
            torch.cuda.synchronize()
            continue
        on_device, on_host = device_arm(), host_arm()                   # warm-up, and the bytes to look at
        times = {'device': [], 'host': []}
        while True:                                                     # taking turns; an arm stops once it has its SECONDS and three calls (Pillow takes seconds per call)
            wanted = [(name, arm) for name, arm in (('device', device_arm), ('host', host_arm)) if sum(times[name]) < args.seconds or len(times[name]) < 3]
            if not wanted:
                break
            for name, arm in wanted:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        # the stages of the device route
        stages = {}

        def clocked(name, work):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = work()
            torch.cuda.synchronize()
            stages.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
            return result
        for _ in range(5):
            hist = clocked('histogram_ms', lambda: gif.histogram(frames))
            palette = clocked('palette_host_ms', lambda: gif.palette_from_histogram(hist))
            table = clocked('lut_ms', lambda: gif.lut(palette))
            units = clocked('encode_and_fetch_ms', lambda: gif.encode(frames, table, dither='ordered'))
            clocked('assemble_host_ms', lambda: gif.assemble(units, size, size, palette))
        # kbe_gif_encode alone: the launches of a call on buffers that exist, HIP events
        cap = sum(len(u) for u in units)
        scratch = torch.empty(int(gif.load().kbe_gif_scratch_bytes(size, size, n)) // 8 + 1, dtype=torch.int64, device='cuda')
        out = torch.empty(cap, dtype=torch.uint8, device='cuda')
        meta = torch.empty(n + 2, dtype=torch.int64, device='cuda')
        pointers = (ctypes.c_void_p * n)(*[frames.data_ptr() + i * size * size * 3 for i in range(n)])
        kernel_ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gif._call('kbe_gif_encode', pointers, n, size, size, 3 * size, 0, gif.DITHER['ordered'], 4, table.data_ptr(), scratch.data_ptr(), out.data_ptr(), cap, meta.data_ptr(),
                      meta.data_ptr() + 8 * (n + 1), _native._stream())
            e1.record()
            torch.cuda.synchronize()
            kernel_ms.append(e0.elapsed_time(e1))
        shown = Image.open(io.BytesIO(on_device))
        assert shown.n_frames == n and shown.size == (size, size)
        first = frames[0].cpu().numpy().astype(np.float64)

        def psnr(data):
            return float(10.0 * np.log10(255.0 ** 2 / np.mean((np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).astype(np.float64) - first) ** 2)))
        med = {name: float(np.median(t)) for name, t in times.items()}
        line = dict(what='frames in HBM -> an animated GIF on the host', size=size, frames=n, gpu=torch.cuda.get_device_name(0), raw_bytes=n * size * size * 3,
                    device_us_per_frame=1e6 * med['device'] / n, host_us_per_frame=1e6 * med['host'] / n, device_over_host_speedup=med['host'] / med['device'],
                    device_bytes_per_frame=len(on_device) / n, host_bytes_per_frame=len(on_host) / n, calls={name: len(t) for name, t in times.items()},
                    device_stages_ms_per_video={name: float(np.median(t)) for name, t in stages.items()},
                    kbe_gif_encode_kernels_only_ms_per_video={'median': float(np.median(kernel_ms)), 'min': min(kernel_ms)},
                    first_frame_psnr_db={'device': psnr(on_device), 'host': psnr(on_host)})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--format', required=True, choices=['mjpeg', 'png', 'gif'])
    ap.add_argument('--sizes', default='512x64,1024x75', help='SIZExFRAMES, comma separated')
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--quality', type=int, default=92, help='mjpeg')
    ap.add_argument('--threads', type=int, default=16, help='host threads of the host arm')
    ap.add_argument('--gif-width', type=int, default=None, help='gif: also the route at this width (reduced on the GPU), against the full size')
    ap.add_argument('--gif-every', type=int, default=1, help='gif: ... and keeping every so-many-th frame and the last')
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'encode_time.py measures on a GPU'
    K = _native.kernels()
    mjpeg = args.format == 'mjpeg'
    assert not mjpeg or pipeline.jpeg_encoder()[0] == 'native'
    own = (args.quality, 0) if mjpeg else (0,)                      # the entry's integers between the stride and the scratch
    if args.format == 'gif':
        return gif_reduced_main(args) if args.gif_width is not None or args.gif_every != 1 else gif_main(args)
    pipeline.WRITER_THREADS = args.threads
    os.environ.pop('KBE_WRITER_THREADS', None)
    lines = []
    for spec in args.sizes.split(','):
        size, n = (int(v) for v in spec.split('x'))
        frames = photo_like(n, size, torch.device('cuda'))
        pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()

        def device_arm():
            return K.mjpeg_encode(frames, args.quality) if mjpeg else K.png_encode(frames)

        def host_arm():
            pinned.copy_(frames, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = pinned.numpy()
            rows = [host[i] for i in range(n)]
            return pipeline._jpegs(rows, args.quality) if mjpeg else pipeline._on_threads(rows, pipeline.png_bytes)

        if args.profile:
            for _ in range(args.rounds):
                device_arm()
            torch.cuda.synchronize()
            continue
        on_device, on_host = device_arm(), host_arm()                   # warm-up, and the bytes to look at
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
        scratch = torch.empty(int(getattr(K.lib, 'kbe_%s_scratch_bytes' % args.format)(size, size, n)) // 8 + 1, dtype=torch.int64, device='cuda')
        cap = sum(len(s) for s in on_device)
        out = torch.empty(cap, dtype=torch.uint8, device='cuda')
        meta = torch.empty(n + 2, dtype=torch.int64, device='cuda')
        pointers = (ctypes.c_void_p * n)(*[frames.data_ptr() + i * size * size * 3 for i in range(n)])
        kernel_ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = K.encode_raw(args.format, pointers, n, size, size, 3 * size, own, scratch.data_ptr(), out.data_ptr(), cap, meta.data_ptr(), meta.data_ptr() + 8 * (n + 1))
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0
            kernel_ms.append(e0.elapsed_time(e1))
        from PIL import Image
        times_of = {name + '_ms_per_video': {'median': 1e3 * float(np.median(t)), 'min': 1e3 * min(t), 'max': 1e3 * max(t), 'calls': len(t)} for name, t in times.items()}
        line = dict(times_of, size=size, frames=n, host_threads=args.threads, device_over_host_speedup=float(np.median(times['host']) / np.median(times['device'])),
                    device_kernels_only_ms_per_video={'median': float(np.median(kernel_ms)), 'min': min(kernel_ms)}, raw_bytes=n * size * size * 3,
                    gpu=torch.cuda.get_device_name(0))
        host_bytes = sum(len(s) for s in on_host)
        if mjpeg:       # what the restart intervals cost in bytes, and that the picture is there
            first = frames[0].cpu().numpy()
            decoded = np.asarray(Image.open(io.BytesIO(on_device[0])).convert('RGB')).astype(np.float64)
            psnr = 10.0 * np.log10(255.0 ** 2 / max(np.mean((decoded - first) ** 2), 1e-12))
            line.update(what='frames in HBM -> Motion-JPEG streams on the host', quality=args.quality, device_stream_bytes=cap, host_stream_bytes=host_bytes,
                        restart_interval_overhead=cap / host_bytes - 1.0, first_frame_psnr_db=float(psnr))
        else:           # lossless: the first and the last file decode to their frames
            for i in (0, n - 1):
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(on_device[i])).convert('RGB')), frames[i].cpu().numpy())
            line.update(what='frames in HBM -> PNG files on the host', device_file_bytes=cap, host_file_bytes=host_bytes, device_over_host_bytes=cap / host_bytes)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
