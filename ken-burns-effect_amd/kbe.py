"""Command line of the reference's ``kbe.py`` (:42-181), same long options:

    python -m ken_burns_effect_amd.kbe --in image.jpg --out outdir [--dolly] [--write-frames]
        [--inpaint-path P] [--refine-path P] [--estim-path P] [--inpaint-depth P] [--pretrained-refine]
        [--pretrained-estim] [--2d] [--startU/--startV/--endU/--endV/--startW/--startH/--endW/--endH N]
        [--semantics-path vgg19_bn_state_dict.pth]     (new: the reference downloads these weights through torchvision)
        [--allow-random-weights]                       (new: render with seeded weights where a checkpoint is missing instead of failing)
        [--jpeg native|pillow|device]                  (new: who encodes a Motion-JPEG video's frames -- host threads, Pillow, or the GPU: env KBE_JPEG)
        [--png native|device]                          (new: who encodes the PNG frames of --write-frames -- host threads or the GPU: env KBE_PNG)
        [--gif] [--gif-dither none|ordered]            (new: also write 3d_kbe.gif, an animated GIF encoded on the GPU: env KBE_GIF=1, KBE_GIF_DITHER)
        [--gif-width N] [--gif-fps F]                  (new, with --gif: the GIF N pixels wide -- reduced on the GPU, never enlarged -- and at about F
                                                        frames a second, every max(1, round(25 / F))-th frame: env KBE_GIF_WIDTH, KBE_GIF_FPS)
        [--width N]                                    (new: every output -- the video, the PNG frames, the GIF -- N pixels wide, the height by the image's
                                                        aspect ratio: the crop reduced on the GPU by an exact area average, never enlarged, so N is
                                                        at most the crop's width; --gif-width is then at most N: env KBE_WIDTH)
        [--enlarge]                                    (new: with --width, N may exceed the crop's width, up to four times it and 16384 pixels a
                                                        side: the crop is then enlarged on the GPU by an exact integer Catmull-Rom bicubic, in
                                                        one resampling from the crop's patch, for a 1080p or 4K clip; an N within the crop is
                                                        reduced as without it: env KBE_ENLARGE=1.  Measured alone: tools/enlarge_time.py,
                                                        profiles/enlarge.json)
        [--aperture A] [--focus U,V] [--focus-to U,V]  (new: depth of field, a lens blur on the GPU from each frame's depth -- A is the blur radius in
                                                        pixels of a point at infinity, above 0; what lies at the depth of pixel U,V of the photo
                                                        stays sharp (default: the centre of the end window), and with --focus-to the focus is pulled
                                                        to that pixel's depth over the clip: env KBE_APERTURE, KBE_FOCUS, KBE_FOCUS_TO)
        [--shutter F] [--shutter-samples S]            (new: motion blur -- the shutter is open for the share F of a frame interval, above 0 and at
                                                        most 1, and every frame is the mean, taken on the GPU, of S frames rendered at sub-frame
                                                        cameras on the path, S = 2..32, default 8: env KBE_SHUTTER, KBE_SHUTTER_SAMPLES)
        [--y4m]                                        (new: also write 3d_kbe.y4m, the clip as planar Y'CbCr 4:2:0 in a YUV4MPEG2 file for a video
                                                        encoder or player, converted on the GPU: env KBE_Y4M=1)
        [--overlay FILE] [--overlay-at ANCHOR|X,Y] [--overlay-opacity O]
                                                       (new: a watermark -- the picture of FILE, with its alpha, composited on the GPU onto every
                                                        frame where the frames lie, before every output is made of them; at one of top-left, top,
                                                        top-right, left, centre, right, bottom-left, bottom, bottom-right (default) or with its
                                                        top-left pixel at X,Y; O above 0 and at most 1, default 1: env KBE_OVERLAY, KBE_OVERLAY_AT,
                                                        KBE_OVERLAY_OPACITY.  Measured alone, tools/overlay_time.py: a full-frame overlay on 12
                                                        frames of 1024^2 takes 21.8 us, 0.94 of the time of a dissolve of the same frames; a
                                                        640 x 64 caption 8.6 us; a delivered 75-frame 1024^2 video 455 ms against 416 without)
        [--caption TEXT] [--caption-at ANCHOR|X,Y] [--caption-size PX] [--font PATH]
                                                       (new: a caption -- TEXT, which may hold line breaks, in white on a half-transparent plate,
                                                        composited the same way under the watermark; default at the bottom, the font's size
                                                        max(12, frame height // 18) pixels, Pillow's built-in face unless PATH names a TrueType
                                                        file: env KBE_CAPTION, KBE_CAPTION_AT, KBE_CAPTION_SIZE)
        [--overlay-margin M]                           (new: the distance of both layers from the edges their anchors name, default
                                                        max(4, frame width // 32) pixels.  Positions are in frame coordinates, after --width; a
                                                        layer that does not fit inside the frame with its margin is refused)
        [--lut FILE] [--grade brightness=B,contrast=C,saturation=S,gamma=G] [--look mono|sepia] [--lut-strength S]
                                                       (new: colour grading -- a 3D lookup table applied on the GPU, with tetrahedral
                                                        interpolation, to every frame where the frames lie, after width, lens and shutter and
                                                        before a caption or watermark, which are never graded: FILE is a .cube look file (3D,
                                                        domain 0..1; more than 33 nodes per axis are resampled to 33); --grade bakes any
                                                        subset of its keys into such a table, on the encoded values, brightness, contrast and
                                                        saturation 0..4, gamma 0.1..10, each 1 by default; --look is a named one; the finished
                                                        grade is --grade and --look first, then the file's table; S above 0 and at most 1,
                                                        default 1, is how much of it shows: env KBE_LUT, KBE_GRADE, KBE_LOOK, KBE_LUT_STRENGTH.
                                                        Measured alone: tools/grade_time.py, profiles/grade.json)
        [--sharpen AMOUNT[,SIGMA[,THRESHOLD]]]         (new: output sharpening -- an exact integer unsharp mask applied on the GPU to every
                                                        frame where the frames lie, after width, enlargement, lens, shutter and grade, the
                                                        last thing done to the picture, and before a caption or watermark, which are never
                                                        sharpened: the frame minus its Gaussian blur of SIGMA pixels, 0.3..8, default 1, is
                                                        added back AMOUNT times, above 0 and at most 4, wherever it is at least THRESHOLD
                                                        counts, 0..255, default 0: env KBE_SHARPEN.  Measured alone: tools/sharpen_time.py,
                                                        profiles/sharpen.json)

Images are read with PIL (OpenCV is not a dependency); like ``cv2.imread`` the pixels are handed to the
networks in BGR order unless ``--pretrained-estim`` is given (kbe.py:96-98).
"""
import getopt
import math
import sys

import numpy as np
import torch

LONG_OPTIONS = ['in=', 'out=', 'dolly', 'write-frames', 'inpaint-path=', 'refine-path=', 'estim-path=', 'startU=', 'startV=', 'endU=',
                'endV=', 'startW=', 'startH=', 'endW=', 'endH=', 'pretrained-refine', 'pretrained-estim', 'inpaint-depth=', '2d', 'semantics-path=', 'allow-random-weights', 'jpeg=', 'png=', 'gif', 'gif-dither=', 'gif-width=', 'gif-fps=', 'width=', 'aperture=', 'focus=', 'focus-to=', 'shutter=', 'shutter-samples=', 'y4m',
                'overlay=', 'overlay-at=', 'overlay-opacity=', 'caption=', 'caption-at=', 'caption-size=', 'font=', 'overlay-margin=',
                'lut=', 'grade=', 'look=', 'lut-strength=', 'enlarge', 'sharpen=']
LAYER_OPTIONS = ('overlay', 'overlay-at', 'overlay-opacity', 'caption', 'caption-at', 'caption-size', 'font', 'overlay-margin')
GRADE_OPTIONS = ('lut', 'grade', 'look', 'lut-strength')


def parse(argv):
    cfg = {'in': 'images/doublestrike.jpg', 'out': 'images/kbe', 'dolly': False, 'write-frames': False, 'pretrained-refine': False,
           'pretrained-estim': False, '2d': False, 'inpaint-depth': None, 'semantics-path': None, 'allow-random-weights': False, 'jpeg': None, 'png': None, 'gif': False, 'gif-dither': None, 'gif-width': None, 'gif-fps': None, 'width': None, 'aperture': None, 'focus': None, 'focus-to': None, 'shutter': None, 'shutter-samples': None, 'y4m': False,
           'overlay': None, 'overlay-at': None, 'overlay-opacity': None, 'caption': None, 'caption-at': None, 'caption-size': None, 'font': None, 'overlay-margin': None,
           'lut': None, 'grade': None, 'look': None, 'lut-strength': None, 'enlarge': False, 'sharpen': None,
           'inpaint-path': './models/trained/inpainting-color.tar', 'refine-path': './models/trained/disparity-refinement.tar',
           'estim-path': './models/trained/disparity-estimation-no-mask.tar'}
    window = dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH'))
    for option, argument in getopt.getopt(argv, '', LONG_OPTIONS)[0]:
        name = option[2:]
        if name in window:
            if argument != '':
                window[name] = int(argument)
        elif name in ('dolly', 'write-frames', 'pretrained-refine', 'pretrained-estim', '2d', 'allow-random-weights', 'gif', 'y4m', 'enlarge'):
            cfg[name] = True
        elif argument != '' or name == 'caption':                        # (an empty caption is refused below, not passed over)
            cfg[name] = argument
    if cfg['png'] not in (None, 'native', 'device'):
        raise SystemExit('--png %s: native or device' % cfg['png'])
    if cfg['gif-dither'] not in (None, 'none', 'ordered'):
        raise SystemExit('--gif-dither %s: none or ordered' % cfg['gif-dither'])
    for name in ('gif-width', 'gif-fps'):
        if cfg[name] is not None and not cfg['gif']:
            raise SystemExit('--%s %s: only with --gif' % (name, cfg[name]))
    if cfg['gif-width'] is not None:
        if not (cfg['gif-width'].isdigit() and int(cfg['gif-width']) >= 1):
            raise SystemExit('--gif-width %s: a number of pixels, 1 or more' % cfg['gif-width'])
        cfg['gif-width'] = int(cfg['gif-width'])
    if cfg['width'] is not None:
        if not (cfg['width'].isdigit() and int(cfg['width']) >= 1):
            raise SystemExit('--width %s: a number of pixels, 1 or more' % cfg['width'])
        cfg['width'] = int(cfg['width'])
        if cfg['gif-width'] is not None and cfg['gif-width'] > cfg['width']:
            raise SystemExit('--gif-width %d: the frames are %d pixels wide (--width), and the GIF is only ever reduced' % (cfg['gif-width'], cfg['width']))
    if cfg['enlarge'] and cfg['width'] is None:
        raise SystemExit('--enlarge: only with --width')
    if cfg['aperture'] is not None or cfg['focus'] is not None or cfg['focus-to'] is not None:
        from .pipeline import lens_request
        for name in ('focus', 'focus-to'):
            if cfg[name] is not None and cfg['aperture'] is None:
                raise SystemExit('--%s %s: only with --aperture' % (name, cfg[name]))
        try:
            cfg['aperture'], cfg['focus'], cfg['focus-to'] = lens_request(cfg['aperture'], cfg['focus'], cfg['focus-to'])
        except ValueError as e:
            raise SystemExit('--%s' % str(e).replace('_', '-', 1) if str(e).startswith('focus') else '--aperture %s: %s' % (cfg['aperture'], e))
    if cfg['shutter'] is not None or cfg['shutter-samples'] is not None:
        from .pipeline import shutter_request
        if cfg['shutter'] is None:
            raise SystemExit('--shutter-samples %s: only with --shutter' % cfg['shutter-samples'])
        try:
            cfg['shutter'], cfg['shutter-samples'] = shutter_request(cfg['shutter'], cfg['shutter-samples'])
        except ValueError as e:
            raise SystemExit('--shutter-samples %s: %s' % (cfg['shutter-samples'], e) if 'samples' in str(e) else '--shutter %s: %s' % (cfg['shutter'], e))
    try:                                                                # the two layers: checked as far as they can be without a frame
        from .overlay import layers_request
        cfg['layers'] = layers_request(*[cfg[name] for name in LAYER_OPTIONS])
    except ValueError as e:
        raise SystemExit(str(e))
    try:                                                                # the grade: the file read, the table baked and all of it checked
        from .grade import grade_request
        cfg['graded'] = grade_request(*[cfg[name] for name in GRADE_OPTIONS])
    except ValueError as e:
        raise SystemExit(str(e))
    try:                                                                # the sharpening: its three fields checked, the taps made
        from .sharpen import request as sharpen_request
        cfg['sharpened'] = sharpen_request(cfg['sharpen'])
    except ValueError as e:
        raise SystemExit(str(e))
    if cfg['gif-fps'] is not None:
        try:
            cfg['gif-fps'] = float(cfg['gif-fps'])
        except ValueError:
            cfg['gif-fps'] = 0.0
        if not 0.0 < cfg['gif-fps'] < float('inf'):
            raise SystemExit('--gif-fps: frames a second, above 0')
    return cfg, window


def windows_for(width, height, window, dolly):
    """kbe.py:116-146: aspect-ratio completion, defaults, and the sanity asserts."""
    w = dict(window)
    if w['endH'] is not None and w['endW'] is None:
        w['endW'] = int(width * w['endH'] / height)
    if w['endW'] is not None and w['endH'] is None:
        w['endH'] = int(height * w['endW'] / width)
    if w['startH'] is not None and w['startW'] is None:
        w['startW'] = int(width * w['startH'] / height)
    if w['startW'] is not None and w['startH'] is None:
        w['startH'] = int(height * w['startW'] / width)
    if None in w.values():
        print('At least one of the cropping parameters was not defined, using default ones for %s.' % ('dolly effect' if dolly else '3D kbe'))
        if not dolly:
            w.update(startU=width / 2.15, startV=height / 2.15, startW=int(math.floor(0.90 * width)), startH=int(math.floor(0.90 * height)),
                     endU=width / 1.85, endV=height / 1.85, endW=int(math.floor(0.85 * width)), endH=int(math.floor(0.85 * height)))
        else:
            w.update(startU=width / 2, startV=height / 2, startW=int(math.floor(0.8 * width)), startH=int(math.floor(0.8 * height)),
                     endU=width / 2, endV=height / 2, endW=int(math.floor(0.3 * width)), endH=int(math.floor(0.3 * height)))
    assert height >= w['startV'] + w['startH'] / 2 and w['startV'] - w['startH'] / 2 >= 0, 'Start window too tall compared to given center'
    assert width >= w['startU'] + w['startW'] / 2 and w['startU'] - w['startW'] / 2 >= 0, 'Start window too wide compared to given center'
    assert height >= w['endV'] + w['endH'] / 2 and w['endV'] - w['endH'] / 2 >= 0, 'End window too tall compared to given center'
    assert width >= w['endU'] + w['endW'] / 2 and w['endU'] - w['endW'] / 2 >= 0, 'End window too wide compared to given center'
    return {'objectFrom': {'dblCenterU': w['startU'], 'dblCenterV': w['startV'], 'intCropWidth': w['startW'], 'intCropHeight': w['startH']},
            'objectTo': {'dblCenterU': w['endU'], 'dblCenterV': w['endV'], 'intCropWidth': w['endW'], 'intCropHeight': w['endH']}}


def load_image(path, rgb):
    """[1,3,H,W] in 0..1, H and W cropped to multiples of 4 (kbe.py:96-114)"""
    from PIL import Image
    img = np.asarray(Image.open(path).convert('RGB'), dtype=np.uint8)
    if not rgb:
        img = img[:, :, ::-1]           # cv2.imread order
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float() / 255.0
    h, w = t.shape[1] - t.shape[1] % 4, t.shape[2] - t.shape[2] % 4
    return t[:, :h, :w].unsqueeze(0)


def main(argv=None):
    from .pipeline import Pipeline, lens_points, width_size
    torch.set_grad_enabled(False)
    cfg, window = parse(sys.argv[1:] if argv is None else argv)
    if cfg['jpeg'] is not None:
        if cfg['jpeg'] not in ('native', 'pillow', 'device'):
            raise SystemExit('--jpeg %s: native, pillow or device' % cfg['jpeg'])
        import os
        os.environ['KBE_JPEG'] = cfg['jpeg']        # (the writers read the switch where they encode: pipeline.jpeg_encoder)
    if cfg['png'] is not None:
        import os
        os.environ['KBE_PNG'] = cfg['png']          # (... and pipeline.png_encoder)
    image = load_image(cfg['in'], cfg['pretrained-estim'])
    if cfg['gif-width'] is not None and cfg['gif-width'] > image.shape[3] and not cfg['enlarge']:      # (with --enlarge: at most --width, checked by parse)
        raise SystemExit('--gif-width %d: the image is %d pixels wide, and the GIF is only ever reduced' % (cfg['gif-width'], image.shape[3]))
    zoom = windows_for(image.shape[3], image.shape[2], window, cfg['dolly'])
    enlarging = {'enlarge': True} if cfg['enlarge'] else {}
    if cfg['width'] is not None:
        try:                                                                # (before any network is built)
            width_size(cfg['width'], image.shape[3], image.shape[2], zoom, **enlarging)
        except ValueError as e:
            raise SystemExit('--width %d: %s' % (cfg['width'], e))
    if cfg['aperture'] is not None:
        try:                                                                # (before any network is built as well)
            lens_points((cfg['aperture'], cfg['focus'], cfg['focus-to']), image.shape[3], image.shape[2], zoom)
        except ValueError as e:
            raise SystemExit('--%s' % str(e).replace('_', '-', 1))
    if cfg['layers'] is not None:
        from .overlay import layers_for
        try:                                                                # (... and the file read, the caption drawn and both fitted to the frames)
            layers_for(cfg['layers'], *(width_size(cfg['width'], image.shape[3], image.shape[2], zoom, **enlarging) if cfg['width'] is not None else (image.shape[3], image.shape[2])),
                       bgr=not cfg['pretrained-estim'])
        except ValueError as e:
            raise SystemExit(str(e))
    paths = [cfg['estim-path'], cfg['refine-path'], cfg['inpaint-path']] + ([cfg['inpaint-depth']] if cfg['inpaint-depth'] else [])
    pipe = Pipeline(model_paths=paths, dolly=cfg['dolly'], output_frames=cfg['write-frames'], pretrain=cfg['pretrained-refine'], d2=cfg['2d'],
                    semantics_path=cfg['semantics-path'], allow_random_weights=cfg['allow-random-weights'] or None, gif=cfg['gif'] or None, gif_dither=cfg['gif-dither'],
                    gif_width=cfg['gif-width'], gif_fps=cfg['gif-fps'], width=cfg['width'], aperture=cfg['aperture'], focus=cfg['focus'], focus_to=cfg['focus-to'],
                    shutter=cfg['shutter'], shutter_samples=cfg['shutter-samples'], y4m=cfg['y4m'] or None,
                    **{name.replace('-', '_'): cfg[name] for name in LAYER_OPTIONS + GRADE_OPTIONS}, **enlarging,
                    **({} if cfg['sharpen'] is None else {'sharpen': cfg['sharpen']}))
    frames = pipe(image, zoom, cfg['out'], pretrained_estim=cfg['pretrained-estim'])
    print('%d frames of %dx%d written to %s' % (len(frames), frames[0].shape[1], frames[0].shape[0], cfg['out']))


if __name__ == '__main__':
    main()
