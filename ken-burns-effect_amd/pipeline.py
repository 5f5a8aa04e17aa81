"""Image -> disparity -> point cloud -> Ken Burns frames.

Drop-in for ``/root/reference/utils/pipeline.py`` (``Pipeline`` :23-134): same constructor and
``__call__`` arguments.  The front half (:61-100: resize, Semantics + Disparity, Refine, disparity
normalisation, depth, unprojection, ``objectCommon``) runs as stock PyTorch-ROCm modules plus the
HIP unprojection; the frame loop is :func:`ken_burns_effect_amd.common.process_kenburns`.

Differences, on purpose: the unused Mask-RCNN of the reference (:36, deleted at :90) is not built; the ImageNet
weights of ``Semantics`` come from a file (``semantics_path``) instead of a torchvision download;
``cv2.minMaxLoc`` is replaced by :func:`synthetic.depthrange_of`; frames are written with PIL and the
video through an ``ffmpeg`` binary if one is on PATH (OpenCV / moviepy are not dependencies) --
otherwise the ``.mp4`` holds Motion-JPEG (ISO base media file written here, no external encoder).  Returns the frame list.
"""
import collections
import math
import os
import shutil
import subprocess

import numpy as np
import torch

from . import common, synthetic
from .disparity_estimation import Disparity, Semantics
from .disparity_refinement import Refine, RefinePretrained
from .partial_inpainting import Inpaint as PartialInpaint
from .pointcloud_inpainting import Inpaint
from .utils import load_models, resize_image


class Pipeline():
    def __init__(self, model_paths=None, partial_inpainting=False, dolly=False, output_frames=False, pretrain=False, d2=False,
                 device='cuda:0', steps=75, inpaint_dtype=None, semantics_path=None, miopen_find=None, allow_random_weights=None, gif=None, gif_dither=None, gif_width=None, gif_fps=None, width=None, aperture=None, focus=None, focus_to=None, shutter=None, shutter_samples=None, y4m=None,
                 overlay=None, overlay_at=None, overlay_opacity=None, caption=None, caption_at=None, caption_size=None, font=None, overlay_margin=None,
                 lut=None, grade=None, look=None, lut_strength=None, enlarge=None, sharpen=None):
        # gif: also write 3d_kbe.gif, encoded on the GPU (gif.py), beside the video; None: env KBE_GIF=1.  gif_dither: 'ordered' (the
        # default; env KBE_GIF_DITHER) or 'none'.  Opt-in: without it every file is written as before.  gif_width: the GIF's width in pixels, at
        # most the frames' -- reduced on the GPU by an exact area average (area.py), the height follows the aspect ratio; env KBE_GIF_WIDTH.
        # gif_fps: the GIF's frame rate, every max(1, round(25 / gif_fps))-th frame and the last; env KBE_GIF_FPS.  None and no env: the
        # frames' own size, every frame
        self.gif, self.gif_dither, self.gif_width, self.gif_fps = gif, gif_dither, gif_width, gif_fps
        # width: every output -- the video, the PNG frames, the GIF, the frames returned -- that many pixels wide instead of the image's
        # width, the height following the image's aspect ratio: the crop reduced on the GPU by an exact area average (crop_area.py), never
        # enlarged, so at most the crop's size (common.crop_size of the zoom settings); env KBE_WIDTH.  gif_width is then taken against
        # the reduced frames.  None and no env: the image's size, every file as before
        self.width = width
        # enlarge: a width above the crop's is taken, up to four times it: the crop is then enlarged on the GPU by an exact integer bicubic
        # (enlarge.py), straight from the crop's patch and not from the frames of the image's size; a width within the crop is reduced as
        # without the switch; env KBE_ENLARGE=1.  None and no env: a width above the crop's is refused, every file as before
        self.enlarge = enlarge
        # aperture: depth of field -- the blur radius, in pixels of the raw frame, of a point at infinity, above 0 and finite; what lies at the
        # focus depth stays sharp (dof.py, common.render_frames(lens=)); env KBE_APERTURE.  focus = (u, v): the pixel of the photo to focus on
        # (default: the centre of the end window); focus_to = (u, v): the focus is pulled there over the clip, linearly in 1 / depth (default:
        # it stays); env KBE_FOCUS, KBE_FOCUS_TO as "U,V".  The depths are read from the estimated depth.  None and no env: no lens, every
        # file as before
        self.aperture, self.focus, self.focus_to = aperture, focus, focus_to
        # shutter: motion blur -- the share of a frame interval the shutter is open, above 0 and at most 1; every frame is then the mean of
        # shutter_samples (2..32, default 8) frames rendered at sub-frame cameras on the path around its own (shutter.py,
        # common.render_frames(shutter=)); env KBE_SHUTTER, KBE_SHUTTER_SAMPLES.  None and no env: an instantaneous exposure, every file as before
        self.shutter, self.shutter_samples = shutter, shutter_samples
        # y4m: also write 3d_kbe.y4m beside the video -- the clip as planar Y'CbCr 4:2:0 in a YUV4MPEG2 file, the one uncompressed format that
        # video encoders and players read, converted on the GPU (yuv.py); None: env KBE_Y4M=1.  Opt-in: without it every file is written as before
        self.y4m = y4m
        # overlay: the path of a picture file composited onto every frame where the frames lie, in HBM -- a watermark (overlay.py); overlay_at: one
        # of overlay.ANCHORS or "X,Y" (default bottom-right); overlay_opacity: above 0 and at most 1 (default 1).  caption: a text drawn on a
        # plate and composited the same way, under the watermark; caption_at (default bottom); caption_size: the font's pixels (default
        # max(12, frame height // 18)); font: the path of a TrueType file (default: Pillow's built-in face).  overlay_margin: the distance of
        # both from the edges their anchors name (default max(4, frame width // 32)).  All in frame coordinates, after `width`.  env
        # KBE_OVERLAY, KBE_OVERLAY_AT, KBE_OVERLAY_OPACITY, KBE_CAPTION, KBE_CAPTION_AT, KBE_CAPTION_SIZE.  None and no env: no layer, every
        # file as before
        self.overlay, self.overlay_at, self.overlay_opacity, self.overlay_margin = overlay, overlay_at, overlay_opacity, overlay_margin
        self.caption, self.caption_at, self.caption_size, self.font = caption, caption_at, caption_size, font
        # lut: the path of a .cube file, a 3D lookup table applied on the GPU to every frame where the frames lie, in HBM, after width, lens
        # and shutter and before the caption and the watermark, which are never graded (grade.py); grade: "brightness=B,contrast=C,
        # saturation=S,gamma=G", any subset (or a dict of them), baked into such a table; look: 'mono' or 'sepia'; the finished grade is
        # grade and look first, then the file's table.  lut_strength: above 0 and at most 1 (default 1), how much of the grade shows.  env
        # KBE_LUT, KBE_GRADE, KBE_LOOK, KBE_LUT_STRENGTH.  None and no env: no grade, every file as before
        self.lut, self.grade, self.look, self.lut_strength = lut, grade, look, lut_strength
        # sharpen: output sharpening -- "AMOUNT[,SIGMA[,THRESHOLD]]" (or a tuple of them): an exact integer unsharp mask applied on the GPU to
        # every frame where the frames lie, in HBM, after width, enlargement, lens, shutter and grade -- the last thing done to the picture --
        # and before the caption and the watermark, which are never sharpened (sharpen.py); AMOUNT above 0 and at most 4, SIGMA 0.3..8
        # (default 1), THRESHOLD 0..255 (default 0); env KBE_SHARPEN.  None and no env: no sharpening, every file as before
        self.sharpen = sharpen
        self.objectCommon = {'dblFocal': 1024.0 / 2, 'dblBaseline': 120}       # pipeline.py:26-27
        # The networks are four fifths of a video's time, and how fast MIOpen runs their convolutions depends on whether this
        # MACHINE has measured them before (measured, MI355X, profiles/r04_networks.txt): PyTorch's default (immediate) mode on a
        # machine with an empty MIOpen find-db picks by heuristics -- the 1024^2 Inpaint forward takes 21.4 ms, the partial one
        # 22.1; MIOpen's find step (torch.backends.cudnn.benchmark) measures the solvers -- 15.0 / 19.3 ms -- but takes 20-50 s in
        # EVERY process that asks for it; yet once one process has run it, its results sit in MIOpen's user find-db on disk and the
        # immediate mode of every later process picks the measured solvers too: 15.0 / 19.3 ms with a first call of 0.1 s.
        # (channels_last is NOT the answer on this stack: 36.3 instead of 21.4 ms immediate, 17.0 instead of 15.0 with the find.)
        # So ``miopen_find`` = 'auto' (the default; env KBE_MIOPEN_FIND=auto): the first call for an image size this machine
        # has not tuned runs under the find step -- it says so on stderr -- and leaves a marker next to the find-db
        # (~/.cache/kbe: utils.miopen_tuned_once); every later call and process runs in immediate mode on the tuned db.  True / '1':
        # always find (a long-lived server that sees many sizes); False / '0': never (tests, one-off runs that cannot wait).
        if miopen_find is None:
            miopen_find = {'1': True, '0': False}.get(os.environ.get('KBE_MIOPEN_FIND', 'auto'), 'auto')
        self.miopen_find = miopen_find
        if miopen_find is True:
            torch.backends.cudnn.benchmark = True
        self.partial_inpainting, self.dolly, self.output_frames, self.d2 = partial_inpainting, dolly, output_frames, d2
        self.device, self.steps = torch.device(device), steps
        self.moduleSemantics = Semantics().to(self.device).eval()
        self.moduleDisparity = Disparity().to(self.device).eval()
        self.moduleRefine = (RefinePretrained() if pretrain else Refine()).to(self.device).eval()
        self.moduleInpaint = (PartialInpaint() if partial_inpainting else Inpaint()).to(self.device).eval()
        models_list = [{'model': self.moduleDisparity, 'type': 'disparity'}, {'model': self.moduleRefine, 'type': 'refine'},
                       {'model': self.moduleInpaint, 'type': 'inpaint'}]
        paths = list(model_paths) if model_paths else [None, None, None]
        if len(paths) == 4:
            # pipeline.py:53-55 builds a second Inpaint for depth; process_inpaint's two-network branch is
            # broken in the reference (common.py:50-69), so the fourth checkpoint is loaded but unused
            self.moduleInpaintDepth = Inpaint().to(self.device).eval()
            models_list.append({'model': self.moduleInpaintDepth, 'type': 'inpaint'})
        # A missing checkpoint is an ERROR, as in the reference (torch.load of utils.py:206 raises): a video rendered from random
        # weights is garbage that looks like a result.  Benches, tests and smoke runs, which only need the arithmetic, say so:
        # ``allow_random_weights=True`` / --allow-random-weights / env KBE_ALLOW_RANDOM_WEIGHTS=1 -> seeded weights and a warning.
        if allow_random_weights is None:
            allow_random_weights = os.environ.get('KBE_ALLOW_RANDOM_WEIGHTS') == '1'
        load_models(models_list, paths, seed_missing=bool(allow_random_weights))
        # optional reduced-precision GridNet (default fp32 = the reference's arithmetic).  ``inpaint_dtype``
        # torch.bfloat16 / torch.float16, or env KBE_INPAINT_DTYPE=bf16|fp16: the two inpaint passes are 80 % of a
        # video's time and run ~4x faster in bf16; the frames then differ visibly in the last bits of the inpainted
        # regions only (not covered by the parity tests)
        if inpaint_dtype is None:
            inpaint_dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16}.get(os.environ.get('KBE_INPAINT_DTYPE', ''))
        if inpaint_dtype is not None and hasattr(self.moduleInpaint, 'compute_dtype'):
            self.moduleInpaint.compute_dtype = inpaint_dtype
        # Semantics = torchvision's vgg19_bn(pretrained=True) in the reference (disparity_estimation.py:86): an ImageNet
        # checkpoint that torchvision downloads.  Neither torchvision nor the network is a dependency here, so the weights
        # come from a file: ``semantics_path`` / env KBE_SEMANTICS_PATH = a torchvision vgg19_bn state dict
        # (torch.save(torchvision.models.vgg19_bn(weights='IMAGENET1K_V1').state_dict(), path) on any machine).  Without
        # it the module gets seeded random weights -- and says so: a trained Disparity checkpoint fed random semantic
        # features gives a meaningless disparity.
        semantics_path = semantics_path or os.environ.get('KBE_SEMANTICS_PATH')
        if semantics_path and os.path.exists(semantics_path):
            state = torch.load(semantics_path, map_location='cpu')
            self.moduleSemantics.load_torchvision_state_dict(state.get('model_state_dict', state) if isinstance(state, dict) else state)
        elif not allow_random_weights:
            raise FileNotFoundError('semantics (VGG19-bn) weights %r not found: pass semantics_path / --semantics-path / KBE_SEMANTICS_PATH (a torchvision '
                                    'vgg19_bn state dict), or allow_random_weights=True / --allow-random-weights for runs that only need the arithmetic'
                                    % (semantics_path,))
        else:
            import warnings
            warnings.warn('checkpoint %r not found: semantics (VGG19-bn) network runs with seeded random weights; pass '
                          'semantics_path / --semantics-path / KBE_SEMANTICS_PATH (a torchvision vgg19_bn state dict)' % (semantics_path,))
            synthetic.seeded_fill_(self.moduleSemantics, 999)

    @torch.no_grad()
    def estimate(self, tensorImage):
        """pipeline.py:61-100: fills ``self.objectCommon`` from an image [1,3,H,W] in 0..1."""
        oc = self.objectCommon
        tensorImage = tensorImage.to(self.device).contiguous()
        oc['intWidth'], oc['intHeight'] = tensorImage.size(3), tensorImage.size(2)
        resized = resize_image(tensorImage, max_size=int(max(oc['intWidth'], oc['intHeight']) / 2))
        disparity = self.moduleDisparity(resized, self.moduleSemantics(resized))
        if self.d2:
            disparity = torch.ones_like(disparity)
        disparity = self.moduleRefine(tensorImage, disparity)
        low = disparity.min()
        if low < 0.0:
            disparity = disparity - low
        disparity = disparity / disparity.max() * oc['dblBaseline']
        depth = (oc['dblFocal'] * oc['dblBaseline']) / (disparity + 1e-7)
        points = common.depth_to_points(depth, oc['dblFocal'])
        oc['dblDispmin'], oc['dblDispmax'] = disparity.min().item(), disparity.max().item()
        oc['objectDepthrange'] = synthetic.depthrange_of(depth)
        oc['tensorRawPoints'] = points.view(1, 3, -1)
        oc['tensorRawImage'], oc['tensorRawDisparity'], oc['tensorRawDepth'] = tensorImage, disparity, depth
        return oc

    @torch.no_grad()
    def __call__(self, tensorImage, zoom_settings, output_path=None, inpaint_depth=False, pretrained_estim=False):
        with common.on_device_of(getattr(self, 'device', torch.device('cpu'))):      # the C ABI launches on the current device's stream
            return self._run(tensorImage, zoom_settings, output_path, inpaint_depth, pretrained_estim)

    @torch.no_grad()
    def render(self, tensorImage, zoom_settings, bgr=True, layers=True):
        """The clip's frames as a uint8 [steps,H,W,3] tensor in HBM, and nothing written: the frames of _run -- the same plan (plan_clip) and
        the same render (_frames), with the instance's width, lens, shutter, grade, sharpening and layers.  bgr: the image's channel order, B,
        G, R unless the caller fed R, G, B; layers=False: without the instance's caption and watermark.  For callers that go on with the
        frames on the device (slideshow.py)."""
        with common.on_device_of(getattr(self, 'device', torch.device('cpu'))):
            plan = plan_clip(self, tensorImage, zoom_settings, bgr, writing=False, layers=layers)
            return plan.filtered(self._frames(tensorImage, zoom_settings, plan, keep_on_device=True))

    def tuning_tag(self, width, height):
        """What MIOpen is tuned for, once per machine (utils.miopen_tuned_once): this pipeline's networks at this image size."""
        return '%dx%d-%s%s%s' % (width, height, 'partial' if self.partial_inpainting else 'plain', '-dolly' if self.dolly else '',
                                 '-pretrain' if isinstance(self.moduleRefine, RefinePretrained) else '')

    def _frames(self, tensorImage, zoom_settings, plan, keep_on_device, inpaint_depth=False):
        """The one render: the networks (estimate), then the frame loop with the plan's keywords -- each absent unless set, so without a width,
        a lens or a shutter the call is what it always was.  A uint8 [steps,H,W,3] tensor in HBM, or with keep_on_device=False a list of host frames."""
        from .utils import miopen_tuned_once
        auto = getattr(self, 'miopen_find', False) == 'auto'
        with miopen_tuned_once(self.tuning_tag(tensorImage.size(3), tensorImage.size(2)) if auto else '', getattr(self, 'device', 'cpu'), enabled=auto):
            self.estimate(tensorImage)
            if inpaint_depth:
                raise NotImplementedError('two-network depth inpainting is broken in the reference (common.py:50-69)')
            return common.process_kenburns({'dblSteps': np.linspace(0.0, 1.0, self.steps).tolist(),
                                            'objectFrom': zoom_settings['objectFrom'], 'objectTo': zoom_settings['objectTo'],
                                            'boolInpaint': True, 'dolly': self.dolly}, self.objectCommon, self.moduleInpaint, keep_on_device=keep_on_device,
                                           **plan.keywords(self.objectCommon))

    def _run(self, tensorImage, zoom_settings, output_path, inpaint_depth, pretrained_estim):
        bgr = not pretrained_estim          # (the frames are in the INPUT's channel order: B, G, R from cv2.imread unless --pretrained-estim)
        plan = plan_clip(self, tensorImage, zoom_settings, bgr, writing=output_path is not None)
        # KBE_JPEG=device, a Motion-JPEG video (no ffmpeg binary) and no PNG frames: the frames stay in HBM, the GPU encodes them and the
        # streams come to the host, a tenth of the pixels' bytes.  KBE_PNG=device and PNG frames asked for: the frames stay in HBM as
        # well and the GPU encodes the PNG files (png_encoder); the video then comes from the same frames in HBM if the first
        # condition holds but for the PNG frames, and from the frames fetched raw otherwise.  The GIF, the y4m file, a grade, a
        # sharpening and a layer keep the frames in HBM too.  Any other combination takes the host route below
        jpeg_on_device = output_path is not None and mjpeg_from_hbm()
        png = output_path is not None and bool(self.output_frames)
        png_on_device = png and png_encoder() == 'device'
        video_from_hbm = jpeg_on_device and (png_on_device or not png)
        on_device = png_on_device or video_from_hbm or plan.gif is not None or plan.y4m or bool(plan.layers) or plan.grade is not None or plan.sharpen is not None
        frames = self._frames(tensorImage, zoom_settings, plan, on_device, inpaint_depth)
        if on_device:                       # (output_path None: only with a grade, a sharpening or a layer, and nothing is written)
            return write_outputs(plan.filtered(frames), output_path, '3d_kbe', bgr, True, png, plan.gif, getattr(self, 'gif_dither', None), plan.y4m, video_from_hbm)
        if output_path is not None:
            os.makedirs(output_path, exist_ok=True)
            # channel order on disk as the reference produces it: frames are in the INPUT's channel order
            # (BGR from cv2.imread unless --pretrained-estim); cv2.imwrite / moviepy want BGR / RGB (:125-134)
            to_rgb = (lambda f: f) if pretrained_estim else (lambda f: f[:, :, ::-1])
            rgb = [to_rgb(f) for f in frames]
            if self.output_frames:
                write_frames(os.path.join(output_path, 'frames'), rgb)
            # forth and back (:131): the SAME array objects twice -- an intra-frame encoder (the Motion-JPEG writers below) encodes each once
            write_video(os.path.join(output_path, '3d_kbe.mp4'), rgb + rgb[-2::-1], fps=25)
        return frames


WRITER_THREADS = None        # host threads the writers encode on (None: one per core, at most 32; KBE_WRITER_THREADS overrides; 1: the caller's thread only)
_JPEG_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'libkbe_jpeg.so')
_JPEG_HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_jpeg.h')
_jpeg_lib = None


def _writer_pool_size(n_jobs):
    want = os.environ.get('KBE_WRITER_THREADS') or WRITER_THREADS or min(32, os.cpu_count() or 1)
    return max(1, min(int(want), max(n_jobs, 1)))


def jpeg_encoder():
    """'native' (libkbe_jpeg.so, include/kbe_jpeg.h: a batch of frames on host threads) or 'pillow' (one frame at a time: Pillow's encoder
    holds the interpreter lock -- measured, 8 threads: 201 ms against 171 ms on one).  KBE_JPEG=pillow forces the latter; a missing
    library falls back to it with a warning (the writers are host-side conveniences, not the render path: that one has no fallback).
    KBE_JPEG=device: the GPU encodes (kbe_mjpeg_encode, include/kbe.h; the second item is then the kernel set, whose mjpeg_encode takes
    frames in HBM) -- opt-in; the same picture with restart intervals in its stream.  No fallback: without the HIP library it raises."""
    global _jpeg_lib
    if os.environ.get('KBE_JPEG', 'native') == 'pillow':
        return 'pillow', None
    if os.environ.get('KBE_JPEG', 'native') == 'device':
        from . import _native
        return 'device', _native.kernels()
    if _jpeg_lib is None:
        import ctypes
        if not os.path.exists(_JPEG_LIB_PATH):
            import warnings
            warnings.warn('%s is missing (python -c "import __graft_entry__ as g; g.build()"): the video writer encodes with Pillow, one frame at a time' % _JPEG_LIB_PATH)
            return 'pillow', None
        from . import _cabi
        _jpeg_lib = _cabi.Header(_JPEG_HEADER_PATH, 'KBE_JPEG_API', 'include/kbe_jpeg.h', library='libkbe_jpeg.so').bind(ctypes.CDLL(_JPEG_LIB_PATH))
    return 'native', _jpeg_lib


def _on_threads(jobs, work):
    """work(job) for every job on the writers' pool of host threads (for work that releases the interpreter lock: zlib does)."""
    workers = _writer_pool_size(len(jobs))
    if workers <= 1:
        return [work(j) for j in jobs]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(work, jobs))


def png_bytes(frame_rgb, level=1):
    """One uint8 HxWx3 frame as a PNG (8-bit RGB, every row with the Sub filter, ONE zlib stream at `level`; default 1 = cv2.imwrite's
    default, /root/reference/utils/pipeline.py:125).  Written here rather than through Pillow because zlib.compress releases the
    interpreter lock and Pillow's PNG encoder does not: write_frames encodes a video's frames side by side."""
    import struct
    import zlib
    a = np.ascontiguousarray(frame_rgb)
    h, w = a.shape[:2]
    raw = np.empty((h, 1 + 3 * w), np.uint8)
    raw[:, 0] = 1                                                   # filter type 1 (Sub): each byte minus the byte three to its left
    flat = a.reshape(h, 3 * w)
    raw[:, 1:4] = flat[:, :3]
    raw[:, 4:] = flat[:, 3:] - flat[:, :-3]                         # (uint8 arithmetic wraps: exactly the filter's modulo 256)

    def chunk(tag, body):
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + chunk(b'IEND', b''))


def png_encoder():
    """Who encodes the PNG frames of --write-frames: 'native' (png_bytes on the writers' host threads, the default) or 'device' (env
    KBE_PNG=device, kbe.py --png device: the GPU encodes frames that stay in HBM -- kbe_png_encode, include/kbe.h --, opt-in; the files are
    lossless either way, their bytes differ).  No fallback: without the HIP library the device route raises."""
    kind = os.environ.get('KBE_PNG', 'native')
    if kind not in ('native', 'device'):
        raise ValueError('KBE_PNG=%s: native or device' % kind)
    return kind


def gif_switch(gif=None):
    """Whether 3d_kbe.gif is written beside the video: what Pipeline was told, else env KBE_GIF=1 (kbe.py --gif).  Off by default."""
    return bool(gif) if gif is not None else os.environ.get('KBE_GIF', '0') == '1'


def y4m_switch(y4m=None):
    """Whether 3d_kbe.y4m is written beside the video: what Pipeline was told, else env KBE_Y4M=1 (kbe.py --y4m).  Off by default."""
    return bool(y4m) if y4m is not None else os.environ.get('KBE_Y4M', '0') == '1'


def gif_dither(kind=None):
    """The GIF's dither: 'ordered' (an 8 x 8 Bayer matrix of one 5-bit step, the default) or 'none'; env KBE_GIF_DITHER, kbe.py --gif-dither."""
    kind = kind or os.environ.get('KBE_GIF_DITHER', 'ordered')
    if kind not in ('none', 'ordered'):
        raise ValueError('KBE_GIF_DITHER=%s: none or ordered' % kind)
    return kind


def gif_shape(width=None, fps=None):
    """(the GIF's width or None for the frames' own, every how many frames it keeps): what Pipeline was told, else env KBE_GIF_WIDTH and
    KBE_GIF_FPS (kbe.py --gif-width, --gif-fps).  The video has 25 frames a second: a GIF of F a second keeps every max(1, round(25 / F))-th."""
    width = width if width is not None else os.environ.get('KBE_GIF_WIDTH') or None
    fps = fps if fps is not None else os.environ.get('KBE_GIF_FPS') or None
    if width is not None:
        try:
            width = int(width)
        except ValueError:
            width = 0
        if width < 1:
            raise ValueError("the GIF's width (KBE_GIF_WIDTH, --gif-width): a number of pixels, 1 or more")
    every = 1
    if fps is not None:
        try:
            fps = float(fps)
        except ValueError:
            fps = 0.0
        if not 0.0 < fps < float('inf'):
            raise ValueError("the GIF's frame rate (KBE_GIF_FPS, --gif-fps): frames a second, above 0")
        every = max(1, int(round(25.0 / fps)))
    return width, every


def layers_of(pipe, size, bgr=True):
    """The layers of a Pipeline for frames of `size` = (W, H), or a function that gives it and is asked only with a layer, in the order they
    are applied -- the caption, then the watermark -- (overlay.layers_for): what it was told, else the environment's twins; [] without
    either.  ValueError whose text begins with the option at fault."""
    from . import overlay
    request = overlay.layers_request(*[getattr(pipe, name, None) for name in overlay.OPTIONS])
    if request is None:
        return []
    W, H = size() if callable(size) else size
    return overlay.layers_for(request, int(W), int(H), bgr)


def grade_of(pipe, bgr=True):
    """The grade of a Pipeline for frames in the channel order bgr (grade.grade_for): what it was told, else the environment's twins -- read,
    checked and baked here, on the host, before any network runs; None without one.  ValueError whose text begins with the option at fault."""
    from . import grade
    return grade.grade_for(grade.grade_request(*[getattr(pipe, name, None) for name in grade.OPTIONS]), bgr)


def sharpen_of(pipe):
    """The sharpening of a Pipeline (sharpen.request): what it was told, else the environment's KBE_SHARPEN -- read and checked on the host;
    None without it."""
    from . import sharpen
    return sharpen.request(getattr(pipe, 'sharpen', None))


def with_sharpen(request, frames):
    """The frames, a uint8 [n,H,W,3] tensor in HBM, sharpened in place (sharpen.apply_sharpen); without a request they are returned as they are."""
    if request is not None:
        from . import sharpen
        sharpen.apply_sharpen(frames, request)
    return frames


def with_grade(graded, frames):
    """The frames, a uint8 [n,H,W,3] tensor in HBM, graded in place (grade.apply_grade); without a grade they are returned as they are."""
    if graded is not None:
        from . import grade
        grade.apply_grade(frames, graded)
    return frames


def with_layers(layers, frames):
    """The frames, a uint8 [n,H,W,3] tensor in HBM, with every layer composited onto every one of them in place (overlay.apply_layers); without a
    layer: as they are."""
    if layers:
        from . import overlay
        overlay.apply_layers(frames, layers)
    return frames


def out_width(width=None):
    """The width of every output in pixels, or None for the image's own: what Pipeline was told, else env KBE_WIDTH (kbe.py --width)."""
    width = width if width is not None else os.environ.get('KBE_WIDTH') or None
    if width is not None:
        try:
            whole = int(width)
            width = whole if whole == float(width) else 0
        except (TypeError, ValueError):
            width = 0
        if width < 1:
            raise ValueError("the outputs' width (KBE_WIDTH, --width): a number of pixels, 1 or more")
    return width


def enlarge_switch(enlarge=None):
    """Whether a width above the crop's is taken, the crop then enlarged (enlarge.py): what Pipeline was told, else env KBE_ENLARGE=1
    (kbe.py --enlarge).  Off by default."""
    return bool(enlarge) if enlarge is not None else os.environ.get('KBE_ENLARGE', '0') == '1'


ENLARGE_FOLD = 4          # the widest output of the switch, in crop widths


def grows(size, zoom_settings):
    """Whether outputs of this (w, h) are larger than the crop of the zoom settings on a side: the frames are then enlarged, not reduced."""
    crop_w, crop_h = (int(v) for v in common.crop_size(zoom_settings))
    return size[0] > crop_w or size[1] > crop_h


def width_size(width, W, H, zoom_settings, enlarge=False):
    """(w, h) of outputs `width` wide from a W x H image: the height follows the image's aspect ratio (crop_area.size_for).  The frames are
    the crop of the zoom settings (common.crop_size) reduced, never enlarged: a width, or its height, above the crop's is refused.
    With ``enlarge`` a width above the crop's is taken, up to ENLARGE_FOLD times it and 16384 pixels a side: the crop is then enlarged
    (grows); one that lets one side grow and the other shrink -- by rounding, near the crop's own size -- is refused."""
    from . import crop_area
    crop_w, crop_h = (int(v) for v in common.crop_size(zoom_settings))
    if enlarge:
        from . import enlarge as enlarge_of
        if width > ENLARGE_FOLD * crop_w:
            raise ValueError('the crop is %d pixels wide: outputs are enlarged at most %d-fold, to %d' % (crop_w, ENLARGE_FOLD, ENLARGE_FOLD * crop_w))
        w, h = enlarge_of.size_for(W, H, width)
        if (w > crop_w and h < crop_h) or (w < crop_w and h > crop_h):
            raise ValueError('the outputs are then %dx%d and the crop is %dx%d: one side would grow and the other shrink' % (w, h, crop_w, crop_h))
        if (w > crop_w or h > crop_h) and max(w, h) > enlarge_of.MAX_SIDE:
            raise ValueError('the outputs are then %dx%d: an enlarged side is at most %d pixels' % (w, h, enlarge_of.MAX_SIDE))
        return w, h
    if width > crop_w:
        raise ValueError('the crop is %d pixels wide: outputs are only ever reduced' % crop_w)
    w, h = crop_area.size_for(W, H, width=width)
    if h > crop_h:
        raise ValueError('the outputs are then %d pixels high and the crop is %d pixels high: outputs are only ever reduced' % (h, crop_h))
    return w, h


def _focus_point(value, what):
    """(u, v) of "U,V" or a pair, or ValueError."""
    try:
        u, v = (value.split(',') if isinstance(value, str) else value)
        u, v = float(u), float(v)
        if not (math.isfinite(u) and math.isfinite(v)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError('%s %s: U,V, a pixel of the photo' % (what, value if isinstance(value, str) else (value,))) from None
    return u, v


def lens_request(aperture=None, focus=None, focus_to=None):
    """(aperture, focus or None, focus_to or None), the points as (u, v), or None for no lens: what Pipeline was told, else env KBE_APERTURE,
    KBE_FOCUS, KBE_FOCUS_TO (kbe.py --aperture, --focus, --focus-to).  The aperture is pixels, above 0 and finite; a focus point without an
    aperture is refused."""
    aperture = aperture if aperture is not None else os.environ.get('KBE_APERTURE') or None
    focus = focus if focus is not None else os.environ.get('KBE_FOCUS') or None
    focus_to = focus_to if focus_to is not None else os.environ.get('KBE_FOCUS_TO') or None
    if aperture is None:
        for value, what in ((focus, 'focus (KBE_FOCUS, --focus)'), (focus_to, 'focus_to (KBE_FOCUS_TO, --focus-to)')):
            if value is not None:
                raise ValueError('%s: only with an aperture (KBE_APERTURE, --aperture)' % what)
        return None
    try:
        aperture = float(aperture)
    except (TypeError, ValueError):
        aperture = 0.0
    if not (math.isfinite(aperture) and aperture > 0.0):
        raise ValueError('the aperture (KBE_APERTURE, --aperture): pixels, a finite number above 0')
    return aperture, None if focus is None else _focus_point(focus, 'focus'), None if focus_to is None else _focus_point(focus_to, 'focus_to')


def shutter_request(shutter=None, samples=None):
    """shutter.Shutter(fraction, samples), or None for an instantaneous exposure: what Pipeline was told, else env KBE_SHUTTER,
    KBE_SHUTTER_SAMPLES (kbe.py --shutter, --shutter-samples).  The fraction is finite, above 0 and at most 1; the samples are an integer 2..32,
    8 where none is given; samples without a shutter are refused."""
    from .shutter import MAX_SAMPLES, Shutter
    shutter = shutter if shutter is not None else os.environ.get('KBE_SHUTTER') or None
    samples = samples if samples is not None else os.environ.get('KBE_SHUTTER_SAMPLES') or None
    if shutter is None:
        if samples is not None:
            raise ValueError('shutter_samples (KBE_SHUTTER_SAMPLES, --shutter-samples): only with a shutter (KBE_SHUTTER, --shutter)')
        return None
    try:
        shutter = float(shutter)
    except (TypeError, ValueError):
        shutter = 0.0
    if not (math.isfinite(shutter) and 0.0 < shutter <= 1.0):
        raise ValueError('the shutter (KBE_SHUTTER, --shutter): the share of a frame interval it is open, a finite number above 0 and at most 1')
    if samples is None:
        return Shutter(shutter)
    try:
        whole = int(samples)
        samples = whole if whole == float(samples) and not isinstance(samples, bool) else 0
    except (TypeError, ValueError, OverflowError):
        samples = 0
    if not 2 <= samples <= MAX_SAMPLES:
        raise ValueError('the shutter\'s samples (KBE_SHUTTER_SAMPLES, --shutter-samples): a whole number, 2..%d' % MAX_SAMPLES)
    return Shutter(shutter, samples)


def lens_points(request, W, H, zoom_settings):
    """(aperture, (u, v) of the first frame's focus, (u, v) of the last frame's) from lens_request's answer for a W x H image, or None.  The
    default focus is the centre of the end window; the default focus_to is the focus.  A point outside the image is refused."""
    if request is None:
        return None
    aperture, focus, focus_to = request
    if focus is None:
        focus = (float(zoom_settings['objectTo']['dblCenterU']), float(zoom_settings['objectTo']['dblCenterV']))
    if focus_to is None:
        focus_to = focus
    for (u, v), what in ((focus, 'focus'), (focus_to, 'focus_to')):
        if not (0.0 <= u <= W - 1 and 0.0 <= v <= H - 1):
            raise ValueError('%s %g,%g: the image is %dx%d: a pixel of the photo, 0..%d and 0..%d' % (what, u, v, W, H, W - 1, H - 1))
    return aperture, focus, focus_to


class ClipPlan(collections.namedtuple('ClipPlan', 'out_size grow lens_at shutter layers grade sharpen gif y4m')):
    """What plan_clip decides about a clip on the host, before any network runs.  out_size: (w, h) of every output, or None for the image's;
    grow: the crop is enlarged to it, not reduced; lens_at: lens_points' answer or None; shutter: a shutter.Shutter or None; layers: the caption
    and the watermark, fitted to the frames ([] without either); grade, sharpen: grade_of's and sharpen_of's answers or None; gif: (its width
    or None for the frames' own, every how many frames it keeps), or None where no GIF is written; y4m: whether the y4m file is."""
    __slots__ = ()

    def keywords(self, estimated):
        """process_kenburns' keywords: out_size, enlarge, lens and shutter, each absent unless set.  estimated: Pipeline.estimate's
        objectCommon -- the lens reads its focus depths from the estimated depth, and nothing else looks at it."""
        keywords = {} if self.out_size is None else {'out_size': self.out_size}
        if self.grow:
            keywords['enlarge'] = True
        if self.lens_at is not None:
            from . import dof
            aperture, near, far = self.lens_at
            keywords['lens'] = dof.Lens(dof.focus_depth(estimated['tensorRawDepth'], *near), dof.focus_depth(estimated['tensorRawDepth'], *far), aperture)
        if self.shutter is not None:
            keywords['shutter'] = self.shutter
        return keywords

    def filtered(self, frames):
        """The frames, a uint8 [n,H,W,3] tensor in HBM, in place: graded, then sharpened -- the last thing done to the picture itself --, then
        under the caption and the watermark, which are neither graded nor sharpened.  Before every output."""
        return with_layers(self.layers, with_sharpen(self.sharpen, with_grade(self.grade, frames)))


def plan_clip(pipe, image, zoom_settings, bgr, writing, layers=True):
    """The ClipPlan of a Pipeline for an image [1,3,H,W] -- of which only the size is read, and only for an option that needs it -- under these
    windows: every option read (what the instance was told, else the environment's twin: the readers above), checked and made ready -- the
    layers' files read and drawn, the grade's table baked -- on the host, before any network runs.  bgr: the frames' channel order, for the layers and the grade; writing: files are written, so the GIF and the y4m file are
    looked at; layers=False: without the instance's caption and watermark.  ValueError for the first fault found, in this order."""
    def told(name):
        return getattr(pipe, name, None)

    def size():
        return int(image.size(3)), int(image.size(2))
    enlarging = enlarge_switch(told('enlarge'))                     # (a width above the crop's is then taken, and the crop enlarged: enlarge.py)
    gif = gif_shape(told('gif_width'), told('gif_fps')) if writing and gif_switch(told('gif')) else None
    if gif is not None and gif[0] is not None and gif[0] > size()[0] and not enlarging:      # (enlarged frames may be wider: see below)
        raise ValueError('a GIF %d pixels wide from an image %d wide: the GIF is only ever reduced' % (gif[0], size()[0]))
    wide, out_size = out_width(told('width')), None
    if wide is not None:
        try:
            out_size = width_size(wide, *size(), zoom_settings, **({'enlarge': True} if enlarging else {}))
        except ValueError as e:
            raise ValueError('width %d: %s' % (wide, e)) from None
        if gif is not None and gif[0] is not None and gif[0] > out_size[0]:
            raise ValueError('a GIF %d pixels wide from frames %d wide: the GIF is only ever reduced' % (gif[0], out_size[0]))
    elif enlarging:
        raise ValueError('enlarge (KBE_ENLARGE, --enlarge): only with a width')
    # (the lens's focus POINTS: its focus depths are read from the estimated depth, in ClipPlan.keywords)
    lens_at = lens_request(told('aperture'), told('focus'), told('focus_to'))
    if lens_at is not None:
        lens_at = lens_points(lens_at, *size(), zoom_settings)
    shutter = shutter_request(told('shutter'), told('shutter_samples'))
    return ClipPlan(out_size, out_size is not None and grows(out_size, zoom_settings), lens_at, shutter,
                    layers_of(pipe, out_size or size, bgr) if layers else [], grade_of(pipe, bgr), sharpen_of(pipe),
                    gif, writing and y4m_switch(told('y4m')))


def mjpeg_from_hbm():
    """Whether the video is Motion-JPEG encoded on the GPU from frames that lie in HBM: no ffmpeg binary, and KBE_JPEG=device."""
    return shutil.which('ffmpeg') is None and jpeg_encoder()[0] == 'device'


def write_outputs(frames, out_dir, stem, bgr, back, png, gif, dither, y4m, video_from_hbm):
    """Every output of frames that lie in HBM, a uint8 [n,H,W,3] tensor in the channel order bgr, as out_dir/stem.mp4 and, where asked for,
    frames/*.png (png), stem.gif (gif: ClipPlan's (width, every); dither: gif_dither's argument) and stem.y4m (y4m) -> the frames as a list
    of host arrays, fetched once.  The device goes first -- the PNG files under KBE_PNG=device, the GIF, the y4m file, the video where
    video_from_hbm (mjpeg_from_hbm, or less: the caller's decision) --, then the fetch, then the host writes what the device did not.
    back: the clip plays forth and back in every stream (pipeline.py:131).  out_dir None: nothing is written."""
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        to_and_fro = {} if back else {'back': False}
        png_on_device = png and png_encoder() == 'device'
        if png_on_device:
            from . import _native
            write_frames(os.path.join(out_dir, 'frames'), None, pngs=_native.kernels().png_encode(frames, bgr=bgr))
        if gif is not None:
            from . import area, gif as gif_of
            size = None if gif[0] is None else area.size_for(frames.shape[2], frames.shape[1], width=gif[0])
            gif_of.write_gif(os.path.join(out_dir, stem + '.gif'), frames, fps=25, bgr=bgr, dither=gif_dither(dither), size=size, every=gif[1], **to_and_fro)
        if y4m:
            from . import yuv
            yuv.write_y4m(os.path.join(out_dir, stem + '.y4m'), frames, fps=25, bgr=bgr, **to_and_fro)
        if video_from_hbm:
            # (every distinct frame is encoded once: the way back is the same byte objects again)
            encoded = jpeg_encoder()[1].mjpeg_encode(frames, 92, bgr=bgr)
            write_video(os.path.join(out_dir, stem + '.mp4'), None, fps=25, jpegs=encoded + encoded[-2::-1] if back else encoded, frame_size=tuple(frames.shape[1:3]))
    host = frames.cpu().numpy()                                     # the one fetch (with video_from_hbm: after the video is written)
    out = [host[i] for i in range(host.shape[0])]
    if out_dir is not None and (png and not png_on_device or not video_from_hbm):
        rgb = [f[:, :, ::-1] for f in out] if bgr else out
        if png and not png_on_device:
            write_frames(os.path.join(out_dir, 'frames'), rgb)
        if not video_from_hbm:
            write_video(os.path.join(out_dir, stem + '.mp4'), rgb + rgb[-2::-1] if back else rgb, fps=25)
    return out


def write_frames(frames_dir, frames_rgb, pngs=None):
    """%d.png per frame (pipeline.py:122-126), encoded on the writers' threads.  ``pngs``: files that are encoded already (one bytes object
    per frame: HipKernels.png_encode); frames_rgb is then not looked at and the writers' threads only write."""
    os.makedirs(frames_dir, exist_ok=True)

    def save(job):
        idx, frame = job
        with open(os.path.join(frames_dir, '%d.png' % idx), 'wb') as f:
            f.write(frame if pngs is not None else png_bytes(frame))
    _on_threads(list(enumerate(pngs if pngs is not None else frames_rgb)), save)


def _encoded(frames_rgb, quality, jpegs, frame_size):
    """(the streams, (h, w)) of a writer's call: pre-encoded ``jpegs`` (one bytes object per frame, with ``frame_size`` = (h, w)), or the
    frames encoded here."""
    if jpegs is not None:
        if frame_size is None or not len(jpegs):
            raise ValueError('pre-encoded jpegs= need frame_size=(h, w) and at least one frame')
        return list(jpegs), (int(frame_size[0]), int(frame_size[1]))
    return _jpegs(frames_rgb, quality), tuple(frames_rgb[0].shape[:2])


def write_mjpeg_avi(path, frames_rgb, fps=25, quality=92, jpegs=None, frame_size=None):
    """A playable video without any external encoder: Motion-JPEG in an AVI container (RIFF 'AVI ' with one 'vids' / 'MJPG' stream,
    an 'idx1' index; every frame a baseline JPEG from PIL).  What write_video writes for an ``.avi`` where there is no ffmpeg binary.
    ``jpegs`` / ``frame_size``: frames that are encoded already (_encoded); frames_rgb is then not looked at."""
    import struct
    jpegs, (h, w) = _encoded(frames_rgb, quality, jpegs, frame_size)
    n = len(jpegs)
    biggest = max(len(j) for j in jpegs)

    def chunk(tag, data):
        return tag + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')

    def lst(tag, data):
        return b'LIST' + struct.pack('<I', len(data) + 4) + tag + data

    avih = struct.pack('<14I', int(1e6 / fps), biggest * fps, 0, 0x10, n, 0, 1, biggest, w, h, 0, 0, 0, 0)       # AVIF_HASINDEX
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIII', 0, 0, 0, 0, 1, fps, 0, n, biggest, 0xFFFFFFFF, 0) + struct.pack('<4h', 0, 0, w, h)
    strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', w * h * 3, 0, 0, 0, 0)
    hdrl = lst(b'hdrl', chunk(b'avih', avih) + lst(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf)))
    index, offset = [], 4
    for j in jpegs:
        index.append(b'00dc' + struct.pack('<III', 0x10, offset, len(j)))               # AVIIF_KEYFRAME
        offset += 8 + len(j) + (len(j) & 1)
    movi_size = offset                                                                  # 'movi' + the chunks
    idx1 = chunk(b'idx1', b''.join(index))
    riff_size = 4 + len(hdrl) + 8 + movi_size + len(idx1)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', riff_size) + b'AVI ' + hdrl + b'LIST' + struct.pack('<I', movi_size) + b'movi')
        for j in jpegs:                                                                 # (streamed: no copy of the whole video in between)
            f.write(b'00dc' + struct.pack('<I', len(j)))
            f.write(j)
            if len(j) & 1:
                f.write(b'\0')
        f.write(idx1)
    return path


def _jpegs(frames_rgb, quality):
    """One baseline JPEG per frame.  A frame OBJECT that occurs several times in the list (the way back of a forth-and-back video,
    pipeline.py:131) is encoded once; the distinct frames go to libkbe_jpeg.so as one batch on the writers' host threads."""
    distinct, first = [], {}
    for frame in frames_rgb:
        if id(frame) not in first:
            first[id(frame)] = len(distinct)
            distinct.append(frame)
    kind, lib = jpeg_encoder()
    sizes = {f.shape for f in distinct}
    if kind == 'native' and len(sizes) == 1:
        import ctypes
        arrays = [np.ascontiguousarray(f, dtype=np.uint8) for f in distinct]
        h, w = arrays[0].shape[:2]
        cap = int(lib.kbe_jpeg_bound(w, h))
        # (the output buffers are worst-case sized -- 6 MB for a 1024^2 frame -- and reused: batches of at most ~256 MB of them)
        per = max(1, min(len(arrays), (256 << 20) // cap))
        outs = [np.empty(cap, np.uint8) for _ in range(per)]
        encoded = []
        for at in range(0, len(arrays), per):
            part = arrays[at:at + per]
            n = len(part)
            got = (ctypes.c_size_t * n)()
            rc = lib.kbe_jpeg_encode_batch((ctypes.c_void_p * n)(*[a.ctypes.data for a in part]), n, w, h, 3 * w, int(quality),
                                           (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs[:n]]), cap, got, _writer_pool_size(n))
            if rc != 0:
                raise RuntimeError('kbe_jpeg_encode_batch: %d' % rc)
            encoded += [outs[i][:got[i]].tobytes() for i in range(n)]
    elif kind == 'device' and len(sizes) == 1:
        import torch
        # (frames that are on the host already: uploaded as one batch; Pipeline hands the encoder its frames where they lie, in HBM)
        stacked = torch.from_numpy(np.stack([np.ascontiguousarray(f, dtype=np.uint8) for f in distinct]))
        encoded = lib.mjpeg_encode(stacked.cuda(), int(quality))
    else:
        import io
        from PIL import Image

        def encode(frame):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(frame)).save(buf, format='JPEG', quality=quality)
            return buf.getvalue()
        encoded = [encode(f) for f in distinct]
    return [encoded[first[id(frame)]] for frame in frames_rgb]


def write_mjpeg_mp4(path, frames_rgb, fps=25, quality=92, jpegs=None, frame_size=None):
    """An ``.mp4`` without any external encoder: an ISO base media file (ISO/IEC 14496-12) with one video track whose samples are
    baseline JPEGs (PIL) -- sample entry ``mp4v`` with an ``esds`` whose objectTypeIndication is 0x6C, "Visual ISO/IEC 10918-1
    (JPEG)", the registered way of carrying Motion-JPEG in MP4 (what ffmpeg's mp4 muxer writes for ``-c:v mjpeg``; ffmpeg-based
    players, VLC and mpv decode it).  Layout: ftyp, mdat (the samples, one chunk), moov (every sample a sync sample: no stss).
    ``jpegs`` / ``frame_size``: frames that are encoded already (_encoded); frames_rgb is then not looked at."""
    import struct
    jpegs, (h, w) = _encoded(frames_rgb, quality, jpegs, frame_size)
    n, delta = len(jpegs), 512
    timescale = int(fps) * delta
    duration = n * delta

    def box(tag, body):
        return struct.pack('>I', len(body) + 8) + tag + body

    def full(tag, version, flags, body):
        return box(tag, struct.pack('>I', (version << 24) | flags) + body)

    def descriptor(tag, body):
        assert len(body) < 128
        return bytes([tag, len(body)]) + body

    matrix = struct.pack('>9I', 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)
    ftyp = box(b'ftyp', b'isom' + struct.pack('>I', 0x200) + b'isomiso2mp41')
    biggest, total = max(len(j) for j in jpegs), sum(len(j) for j in jpegs)
    first_sample = len(ftyp) + 8
    assert first_sample + total + 8 < (1 << 32), 'a 32-bit chunk offset: the video is too long for this writer'
    decoder = descriptor(0x04, bytes([0x6C, 0x11]) + struct.pack('>I', biggest)[1:] + struct.pack('>II', biggest * 8 * int(fps), total * 8 * int(fps) // n))
    esds = full(b'esds', 0, 0, descriptor(0x03, struct.pack('>HB', 1, 0) + decoder + descriptor(0x06, b'\x02')))
    name = b'Motion-JPEG'
    mp4v = box(b'mp4v', b'\0' * 6 + struct.pack('>H', 1) + b'\0' * 16 + struct.pack('>HHIIIH', w, h, 0x480000, 0x480000, 0, 1) +
               bytes([len(name)]) + name.ljust(31, b'\0') + struct.pack('>Hh', 24, -1) + esds)
    stbl = box(b'stbl', full(b'stsd', 0, 0, struct.pack('>I', 1) + mp4v) +
               full(b'stts', 0, 0, struct.pack('>III', 1, n, delta)) +
               full(b'stsc', 0, 0, struct.pack('>IIII', 1, 1, n, 1)) +
               full(b'stsz', 0, 0, struct.pack('>II', 0, n) + b''.join(struct.pack('>I', len(j)) for j in jpegs)) +
               full(b'stco', 0, 0, struct.pack('>II', 1, first_sample)))
    minf = box(b'minf', full(b'vmhd', 0, 1, struct.pack('>4H', 0, 0, 0, 0)) +
               box(b'dinf', full(b'dref', 0, 0, struct.pack('>I', 1) + full(b'url ', 0, 1, b''))) + stbl)
    mdia = box(b'mdia', full(b'mdhd', 0, 0, struct.pack('>IIIIHH', 0, 0, timescale, duration, 0x55C4, 0)) +
               full(b'hdlr', 0, 0, struct.pack('>I', 0) + b'vide' + b'\0' * 12 + b'VideoHandler\0') + minf)
    tkhd = full(b'tkhd', 0, 3, struct.pack('>IIIII', 0, 0, 1, 0, duration) + b'\0' * 8 + struct.pack('>hhhH', 0, 0, 0, 0) + matrix +
                struct.pack('>II', w << 16, h << 16))
    mvhd = full(b'mvhd', 0, 0, struct.pack('>IIIIIH', 0, 0, timescale, duration, 0x10000, 0x100) + b'\0' * 10 + matrix + b'\0' * 24 + struct.pack('>I', 2))
    with open(path, 'wb') as f:
        # (the samples go out one by one: joined into one `mdat` body first, then into one file image, the video's 20 MB were copied three
        # times before they reached the file -- more than half of what the writer took once the encoding ran on threads)
        f.write(ftyp + struct.pack('>I', total + 8) + b'mdat')
        for j in jpegs:
            f.write(j)
        f.write(box(b'moov', mvhd + box(b'trak', tkhd + mdia)))
    return path


def write_video(path, frames_rgb, fps=25, jpegs=None, frame_size=None):
    """mpeg4 through an ffmpeg pipe when the binary exists (what moviepy does, pipeline.py:132-134).  Without one the video is still
    written, under the name asked for, with the encoder this package carries: Motion-JPEG -- in an MP4 container for an ``.mp4``
    (write_mjpeg_mp4), in an AVI for an ``.avi`` (write_mjpeg_avi) -- and the function says so and returns False.  ``jpegs`` /
    ``frame_size``: the frames as Motion-JPEG streams encoded already (the writers' arguments); only the Motion-JPEG route can take them."""
    ffmpeg = shutil.which('ffmpeg')
    if ffmpeg is None:
        writer = write_mjpeg_avi if path.lower().endswith('.avi') else write_mjpeg_mp4
        writer(path, frames_rgb, fps, jpegs=jpegs, frame_size=frame_size)
        print('ffmpeg not found: %s holds Motion-JPEG (%d frames at %d fps) instead of mpeg4' % (path, len(jpegs if jpegs is not None else frames_rgb), fps))
        return False
    if frames_rgb is None:
        raise ValueError('write_video: pre-encoded jpegs= are Motion-JPEG; the ffmpeg route needs the frames')
    h, w = frames_rgb[0].shape[:2]
    proc = subprocess.Popen([ffmpeg, '-y', '-loglevel', 'error', '-f', 'rawvideo', '-pix_fmt', 'rgb24', '-s', '%dx%d' % (w, h),
                             '-r', str(fps), '-i', '-', '-c:v', 'mpeg4', path], stdin=subprocess.PIPE)
    for frame in frames_rgb:
        proc.stdin.write(np.ascontiguousarray(frame).tobytes())
    proc.stdin.close()
    return proc.wait() == 0
