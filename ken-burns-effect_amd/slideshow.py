"""Slideshows: several photos in one video, every photo a Ken Burns clip, the clips joined on the GPU by transitions (transition.py):

    python -m ken_burns_effect_amd.slideshow --in a.jpg --in b.jpg [--in c.jpg ...] --out outdir
        [--transition dissolve|wipe-right|wipe-left|wipe-down|wipe-up|fade]   (default dissolve)
        [--transition-frames T]                        (default 12: the last T frames of a clip and the first T of the next become T frames)
        [--softness S]                                 (the wipes' soft edge in pixels, 1..65535; default: an eighth of the wipe's extent, at least 1)
        [--fade-colour R,G,B]                          (the colour the fade, --fade-in and --fade-out go through; default 0,0,0)
        [--fade-in N] [--fade-out N]                   (the show's first / last N frames come from / go to the colour; default 0)
        [--caption TEXT] ... [--caption-fade F]        (one --caption per --in, in their order, or none; "" for a photo without one.  A caption
                                                        is composited on the GPU onto its own clip before the clips are joined: it fades in over F
                                                        frames, default 12, and out over F, inside the clip's frames that no transition, --fade-in
                                                        or --fade-out uses, so it is never seen where two clips or the fade colour meet.  Measured
                                                        alone, tools/overlay_time.py: a 640 x 64 caption on 12 frames of 1024^2 takes 8.6 us)
        [--overlay FILE]                               (a watermark on every frame of the joined show, at a constant opacity: it does not dim
                                                        under a fade) with kbe.py's [--overlay-at A] [--overlay-opacity O] [--caption-at A]
                                                        [--caption-size PX] [--font PATH] [--overlay-margin M]
        [--lut FILE] [--grade K=V,...] [--look mono|sepia] [--lut-strength S]
                                                       (kbe.py's colour grading: every clip is graded on the GPU where Pipeline.render leaves it,
                                                        so transitions blend graded frames; the fade colour, the captions and the watermark are
                                                        not graded.  One grade for the whole show)
        [--sharpen AMOUNT[,SIGMA[,THRESHOLD]]]         (kbe.py's output sharpening: every clip is sharpened on the GPU after its grade, before
                                                        the clips are joined; the captions and the watermark are not sharpened.  One setting
                                                        for the whole show)
        and of kbe.py's options: [--dolly] [--width N] [--enlarge] [--aperture A] [--focus U,V] [--focus-to U,V] [--shutter F] [--shutter-samples S]
        [--gif] [--gif-dither none|ordered] [--gif-width N] [--gif-fps F] [--y4m] [--write-frames] [--jpeg native|pillow|device]
        [--png native|device] [--inpaint-path P] [--refine-path P] [--estim-path P] [--inpaint-depth P] [--pretrained-refine]
        [--pretrained-estim] [--2d] [--semantics-path P] [--allow-random-weights]

One Pipeline is built: the networks are loaded once.  Every photo gets kbe.py's default windows (window options are not taken) and its clip
plays forth only; Pipeline.render leaves each clip's frames in HBM, transition.join makes one tensor of them, and the writers take the
frames where they lie: slideshow.mp4 -- encoded on the GPU under KBE_JPEG=device where there is no ffmpeg binary, otherwise the frames are
fetched once for write_video --, and with the switches slideshow.gif, slideshow.y4m and frames/*.png.  All photos must give frames of one
size: the image's, or --width's.
"""
import getopt
import os
import sys

import torch

from . import kbe, overlay, transition

STEPS = 75                # the frames of every clip on the command line (Pipeline's default)
OWN_OPTIONS = ['transition=', 'transition-frames=', 'softness=', 'fade-colour=', 'fade-in=', 'fade-out=', 'caption-fade=']
WINDOW_OPTIONS = ('startU=', 'startV=', 'endU=', 'endV=', 'startW=', 'startH=', 'endW=', 'endH=')
LONG_OPTIONS = [o for o in kbe.LONG_OPTIONS if o not in WINDOW_OPTIONS] + OWN_OPTIONS
NO_WINDOW = dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH'))


def _whole(text):
    """A whole number 0 or more from the command line's text or a number, or None."""
    if isinstance(text, int) and not isinstance(text, bool):
        return text if text >= 0 else None
    return int(text) if isinstance(text, str) and text.isdigit() else None


def colour_bytes(text):
    """(R, G, B) from "R,G,B" or three numbers, 0..255 each, or ValueError."""
    try:
        parts = text.split(',') if isinstance(text, str) else list(text)
        values = [_whole(v.strip() if isinstance(v, str) else v) for v in parts]
    except (TypeError, AttributeError):
        values = []
    if len(values) != 3 or any(v is None or v > 255 for v in values):
        raise ValueError('the fade colour (--fade-colour): R,G,B, three whole numbers 0..255')
    return tuple(values)


def frame_size(W, H, zoom, width=None, enlarge=False):
    """(w, h) of the frames a W x H photo gives under these windows: the photo's size, or --width's (pipeline.width_size; with ``enlarge``
    it may exceed the crop's)."""
    from .pipeline import width_size
    return (int(W), int(H)) if width is None else width_size(width, W, H, zoom, **({'enlarge': True} if enlarge else {}))


def caption_windows(steps, photos, T, fade_in=0, fade_out=0):
    """[(first, last)] per clip: the frames [first, last) of a clip of `steps` that no junction of T frames and no fade uses -- where a caption may show."""
    return [(T if i > 0 else fade_in, steps - (T if i + 1 < photos else fade_out)) for i in range(photos)]


def show_layers(show, request, bgr=True):
    """([per clip: a caption's layer (picture, x, y, its opacities per frame of the clip) or None], the watermark's layer or None) of a checked
    show and the layers' request (overlay.layers_request; None: the defaults): drawn, read and fitted to the frames on the host, before any
    network runs.  ValueError whose text begins with the option at fault."""
    W, H = show['size']
    texts = show['captions'] or []
    if any(texts) and request is None:                              # (captions without a word on where and how large: the defaults)
        request = overlay.layers_request(caption=next(t for t in texts if t), environment=False)
    captions = []
    for text, (first, last) in zip(texts, show['windows']):
        if not text:
            captions.append(None)
            continue
        picture, x, y, peak = overlay.caption_layer(request, text, W, H, bgr)
        captions.append((picture, x, y, overlay.opacity_table(show['steps'], first, last, show['caption_fade'], peak)))
    return captions, overlay.overlay_layer(request, W, H, bgr) if request is not None and request['overlay'] is not None else None


def checked(sizes, steps, transition_kind='dissolve', transition_frames=12, softness=None, fade_colour=(0, 0, 0), fade_in=0, fade_out=0, width=None, dolly=False, names=None,
            captions=None, caption_fade=12, enlarge=False):
    """What a slideshow of photos of these (W, H) sizes will be, from the sizes, the default windows and the width alone -- before any network runs:
    {'size': (w, h) of every frame, 'zooms', 'kind', 'T', 'softness', 'colour': (R, G, B), 'fade_in', 'fade_out', 'plan': transition.join_plan's,
    'steps', 'captions': one text per photo or None, 'caption_fade', 'windows': caption_windows'}, or ValueError whose text begins with the option at fault."""
    names = list(names) if names is not None else ['photo %d' % i for i in range(len(sizes))]
    if enlarge and width is None:
        raise ValueError('--enlarge: only with --width')
    if len(sizes) < 1:
        raise ValueError('--in: a slideshow takes one photo or more')
    if transition_kind not in transition.KINDS:
        raise ValueError('--transition %s: %s' % (transition_kind, ', '.join(transition.KINDS)))
    T, steps = _whole(transition_frames), int(steps)
    if len(sizes) > 1 and not (T is not None and 1 <= T <= steps // 2):
        raise ValueError("--transition-frames %s: 1..%d, half of a clip's %d frames" % (transition_frames, steps // 2, steps))
    if softness is not None and not (_whole(softness) is not None and 1 <= _whole(softness) <= transition.MAX_SOFTNESS):
        raise ValueError("--softness %s: the wipes' soft edge in pixels, 1..%d" % (softness, transition.MAX_SOFTNESS))
    try:
        colour = colour_bytes(fade_colour)
    except ValueError as e:
        raise ValueError('--fade-colour %s: %s' % (fade_colour if isinstance(fade_colour, str) else (fade_colour,), e)) from None
    used = T if len(sizes) > 1 else 0
    for option, value in (('--fade-in', fade_in), ('--fade-out', fade_out)):
        if _whole(value) is None or _whole(value) > steps - used:
            raise ValueError("%s %s: 0..%d, the frames of a clip of %d that no transition uses" % (option, value, steps - used, steps))
    if len(sizes) == 1 and _whole(fade_in) + _whole(fade_out) > steps:
        raise ValueError("--fade-out %s: with --fade-in %s more than the clip's %d frames" % (fade_out, fade_in, steps))
    captions = list(captions) if captions else None
    if captions is not None and (len(captions) != len(sizes) or not all(isinstance(t, str) for t in captions)):
        raise ValueError('--caption: %d captions for %d photos: one per photo, in their order ("" for a photo without one), or none' % (len(captions), len(sizes)))
    windows = caption_windows(steps, len(sizes), used, _whole(fade_in), _whole(fade_out))
    F = _whole(caption_fade)
    narrowest = min([last - first for text, (first, last) in zip(captions or [], windows) if text] or [steps])
    if F is None or (captions is not None and any(captions) and 2 * F > narrowest):
        raise ValueError("--caption-fade %s: 0..%d, half of the %d frames of a captioned clip that no transition or fade uses" % (caption_fade, max(narrowest, 0) // 2, max(narrowest, 0)))
    zooms, size = [], None
    for i, (W, H) in enumerate(sizes):
        zooms.append(kbe.windows_for(W, H, NO_WINDOW, dolly))
        try:
            mine = frame_size(W, H, zooms[-1], width, enlarge)
        except ValueError as e:
            raise ValueError('--width %d: %s: %s' % (width, names[i], e)) from None
        if size is None:
            size = mine
        elif mine != size:
            raise ValueError("--in %s: its frames are %dx%d and %s's are %dx%d: a slideshow's photos give frames of one size (see --width)" % (
                names[i], mine[0], mine[1], names[0], size[0], size[1]))
    kind = transition.KINDS[transition_kind]
    return {'size': size, 'zooms': zooms, 'kind': kind, 'T': used, 'colour': colour, 'fade_in': _whole(fade_in), 'fade_out': _whole(fade_out),
            'softness': _whole(softness) if softness is not None else transition.default_softness(kind, size[0], size[1]),
            'plan': transition.join_plan([steps] * len(sizes), used, _whole(fade_in), _whole(fade_out)),
            'steps': steps, 'captions': captions, 'caption_fade': F, 'windows': windows}


def parse(argv):
    """(cfg of kbe.parse with 'in' a list of paths and the slideshow's own options) from the command line, or SystemExit."""
    try:
        options = getopt.getopt(argv, '', LONG_OPTIONS)[0]
    except getopt.GetoptError as e:
        raise SystemExit('%s%s' % (e, ': window options are not taken, every photo gets the default windows' if str(e.opt) + '=' in WINDOW_OPTIONS else ''))
    own = {'transition': 'dissolve', 'transition-frames': '12', 'softness': None, 'fade-colour': '0,0,0', 'fade-in': '0', 'fade-out': '0', 'caption-fade': '12'}
    images, rest, captions = [], [], []
    for option, argument in options:
        name = option[2:]
        if name == 'in':
            images.append(argument)
        elif name == 'caption':
            captions.append(argument)
        elif name in own:
            own[name] = argument
        else:
            rest += [option] + ([argument] if name + '=' in LONG_OPTIONS else [])
    # (kbe.py checks the layers' options with one caption in the captions' place: the first there is)
    cfg = kbe.parse(rest + (['--caption', next(t for t in captions if t)] if any(captions) else []))[0]
    cfg.update(own)
    cfg['in'], cfg['caption'] = images, captions
    if cfg['layers'] is not None and not any(captions):
        cfg['layers'] = dict(cfg['layers'], caption=None) if cfg['layers']['overlay'] is not None else None     # (KBE_CAPTION is kbe.py's: a slideshow's captions go with its photos)
    if cfg['out'] == 'images/kbe':
        cfg['out'] = 'images/slideshow'
    return cfg


def make(images, out_dir, pipe, transition_kind='dissolve', transition_frames=12, softness=None, fade_colour=(0, 0, 0), fade_in=0, fade_out=0,
         pretrained_estim=False, gif=False, y4m=False, names=None, captions=None, caption_fade=12, layers=None):
    """images: [1,3,H,W] tensors in 0..1, one per photo -> the slideshow's frames as a list of uint8 arrays, written to out_dir (None: nothing
    is written) as slideshow.mp4 and, with gif / y4m / pipe.output_frames, slideshow.gif, slideshow.y4m and frames/*.png.  pipe: the one
    Pipeline whose render makes every clip, pipe.steps frames each, with its width, lens and shutter -- and without its layers, if it has any.
    captions: one text per photo ("" for none), each composited onto its own clip in HBM before the join, fading in and out over caption_fade
    frames inside the clip's frames that no junction and no fade uses; layers: overlay.layers_request's answer -- where and how large the
    captions are, and the watermark, which is composited onto every joined frame at a constant opacity.  ValueError (checked, show_layers)
    before a network runs."""
    from . import pipeline as P
    width = P.out_width(getattr(pipe, 'width', None))
    show = checked([(int(t.shape[3]), int(t.shape[2])) for t in images], pipe.steps, transition_kind, transition_frames, softness, fade_colour, fade_in, fade_out,
                   width=width, dolly=bool(pipe.dolly), names=names, captions=captions, caption_fade=caption_fade, enlarge=P.enlarge_switch(getattr(pipe, 'enlarge', None)))
    bgr = not pretrained_estim                                      # (the frames are in the INPUT's channel order: B, G, R unless --pretrained-estim)
    titles, watermark = show_layers(show, layers, bgr)
    P.grade_of(pipe, bgr)                                           # (the clips' grade, which pipe.render applies: refused here, before a network runs)
    P.sharpen_of(pipe)                                              # (... and their sharpening, which pipe.render applies after the grade)
    gif = P.gif_shape(getattr(pipe, 'gif_width', None), getattr(pipe, 'gif_fps', None)) if out_dir is not None and gif else None
    if gif is not None and gif[0] is not None and gif[0] > show['size'][0]:
        raise ValueError('a GIF %d pixels wide from frames %d wide: the GIF is only ever reduced' % (gif[0], show['size'][0]))
    R, G, B = show['colour']
    # (the layers are the show's: a clip is rendered without the Pipeline's own -- and graded, if the Pipeline has a grade, in the frames' channel order)
    clips = [pipe.render(image, zoom, bgr=bgr, layers=False) for image, zoom in zip(images, show['zooms'])]
    with P.common.on_device_of(pipe.device):
        for clip, title in zip(clips, titles):
            if title is not None:
                P.with_layers([title], clip)
        frames = transition.join(clips, show['kind'], show['T'], show['softness'], (B, G, R) if bgr else (R, G, B), show['fade_in'], show['fade_out'])
        del clips
        if watermark is not None:
            P.with_layers([watermark], frames)
        # (the show plays forth only; its video comes from HBM wherever the GPU encodes it, beside PNG frames written on the host as well)
        return P.write_outputs(frames, out_dir, 'slideshow', bgr, False, out_dir is not None and bool(pipe.output_frames), gif, getattr(pipe, 'gif_dither', None),
                               bool(y4m), out_dir is not None and P.mjpeg_from_hbm())


def main(argv=None):
    from .pipeline import Pipeline
    torch.set_grad_enabled(False)
    cfg = parse(sys.argv[1:] if argv is None else argv)
    if cfg['jpeg'] is not None:
        if cfg['jpeg'] not in ('native', 'pillow', 'device'):
            raise SystemExit('--jpeg %s: native, pillow or device' % cfg['jpeg'])
        os.environ['KBE_JPEG'] = cfg['jpeg']
    if cfg['png'] is not None:
        os.environ['KBE_PNG'] = cfg['png']
    if not cfg['in']:
        raise SystemExit('--in: a slideshow takes one photo or more')
    if cfg['transition'] not in transition.KINDS:                       # (before a file is read)
        raise SystemExit('--transition %s: %s' % (cfg['transition'], ', '.join(transition.KINDS)))
    images = [kbe.load_image(path, cfg['pretrained-estim']) for path in cfg['in']]
    settings = dict(transition_kind=cfg['transition'], transition_frames=cfg['transition-frames'], softness=cfg['softness'], fade_colour=cfg['fade-colour'],
                    fade_in=cfg['fade-in'], fade_out=cfg['fade-out'], captions=cfg['caption'], caption_fade=cfg['caption-fade'])
    try:                                                                # (before any network is built)
        show = checked([(int(t.shape[3]), int(t.shape[2])) for t in images], STEPS, width=cfg['width'], dolly=cfg['dolly'], names=cfg['in'], enlarge=cfg['enlarge'], **settings)
        show_layers(show, cfg['layers'], not cfg['pretrained-estim'])
    except ValueError as e:
        raise SystemExit(str(e))
    if cfg['gif-width'] is not None and cfg['gif-width'] > show['size'][0]:
        raise SystemExit('--gif-width %d: the frames are %d pixels wide, and the GIF is only ever reduced' % (cfg['gif-width'], show['size'][0]))
    if cfg['aperture'] is not None:
        from .pipeline import lens_points
        for image, zoom, path in zip(images, show['zooms'], cfg['in']):
            try:
                lens_points((cfg['aperture'], cfg['focus'], cfg['focus-to']), image.shape[3], image.shape[2], zoom)
            except ValueError as e:
                raise SystemExit('--%s (%s)' % (str(e).replace('_', '-', 1), path))
    paths = [cfg['estim-path'], cfg['refine-path'], cfg['inpaint-path']] + ([cfg['inpaint-depth']] if cfg['inpaint-depth'] else [])
    pipe = Pipeline(model_paths=paths, dolly=cfg['dolly'], output_frames=cfg['write-frames'], pretrain=cfg['pretrained-refine'], d2=cfg['2d'],
                    semantics_path=cfg['semantics-path'], allow_random_weights=cfg['allow-random-weights'] or None, gif_dither=cfg['gif-dither'],
                    gif_width=cfg['gif-width'], gif_fps=cfg['gif-fps'], width=cfg['width'], aperture=cfg['aperture'], focus=cfg['focus'], focus_to=cfg['focus-to'],
                    shutter=cfg['shutter'], shutter_samples=cfg['shutter-samples'], steps=STEPS,
                    **{name.replace('-', '_'): cfg[name] for name in kbe.GRADE_OPTIONS}, **({'enlarge': True} if cfg['enlarge'] else {}),
                    **({} if cfg['sharpen'] is None else {'sharpen': cfg['sharpen']}))
    frames = make(images, cfg['out'], pipe, pretrained_estim=cfg['pretrained-estim'], gif=cfg['gif'], y4m=cfg['y4m'], names=cfg['in'], layers=cfg['layers'], **settings)
    print('%d frames of %dx%d from %d photos written to %s' % (len(frames), frames[0].shape[1], frames[0].shape[0], len(images), cfg['out']))


if __name__ == '__main__':
    main()
