"""Transitions: a frame made of two frames -- a dissolve, a wipe with a soft edge, a fade through a colour --, taken on the GPU from frames that
lie in HBM (include/kbe_transition.h: kbe_transition_u8; the arithmetic is defined in csrc/kbe_transition_block.h), and what a slideshow needs
of them: join puts several clips into one tensor, the frames at every junction made of the last frames of one clip and the first frames of the
next (slideshow.py is its user).  Exact and byte-defined: blend(a, b, w) = (a (256 - w) + b w + 128) >> 8 in integers, w in 0..256.

This is the only module that names the entries of kbe_transition.h: they are exported by libkbe_hip.so beside those of the other headers and
typed from their own header on the package's one handle of that library, the way the other frame filters' modules type their own.  No
fallback: without the HIP library every call here raises.
"""
import ctypes
import os

from . import _cabi, _native

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'kbe_transition.h')
ABI_VERSION = 1
FRAMES_PER_LAUNCH = 12             # KBE_TRANSITION_FRAMES_PER_LAUNCH: the entry cuts a call's frames into launches of this many
MAX_SIDE = 65535
MAX_SOFTNESS = 65535
KINDS = {'dissolve': 0, 'wipe-right': 1, 'wipe-left': 2, 'wipe-down': 3, 'wipe-up': 4, 'fade': 5}
FADE = KINDS['fade']
HEADER = _cabi.Header(HEADER_PATH, 'KBE_TRANSITION_API', 'include/kbe_transition.h', abi=('kbe_transition_abi_version', ABI_VERSION, 'transition '))
prototypes = HEADER.prototypes     # {entry: (restype, [argtypes])} of every entry include/kbe_transition.h declares, in its order, read once


def load():
    """The package's one handle of libkbe_hip.so (_native.load), its transition entries typed from include/kbe_transition.h the first time it is seen."""
    return HEADER.bind(_native.load())


def _raw(name, *args):
    """The entry `name` of include/kbe_transition.h with plain Python values -> what it returns; a surplus argument, which cdecl lets through, is refused."""
    return HEADER.raw(load(), name, *args)


def _call(name, *args):
    """An entry that returns a status: KbeError with the library's text unless KBE_OK."""
    HEADER.call(load(), name, *args)


def progress_table(T):
    """The progress of the T frames of a transition: 256 (j + 1) / (T + 1), rounded half up.  It never holds 0 or 256: a transition frame is
    never a copy of a clip's frame."""
    T = int(T)
    return [(512 * (j + 1) + (T + 1)) // (2 * (T + 1)) for j in range(T)]


def default_softness(kind, W, H):
    """An eighth of the wipe's extent -- the width for the horizontal wipes, the height for the vertical ones --, at least 1."""
    kind = kind_of(kind)
    return max(1, min(MAX_SOFTNESS, (H if kind in (KINDS['wipe-down'], KINDS['wipe-up']) else W) // 8))


def kind_of(kind, what='transition'):
    """The number of a kind given by its name or its number, or ValueError."""
    if isinstance(kind, str) and kind in KINDS:
        return KINDS[kind]
    if isinstance(kind, int) and not isinstance(kind, bool) and kind in KINDS.values():
        return kind
    raise ValueError('%s: kind = %r: one of %s' % (what, kind, ', '.join(KINDS)))


def colour_of(colour, what='transition'):
    """The colour as the entry takes it -- byte k of a pixel meets (colour >> 8 k) & 255 -- from such a number or from the three bytes of a pixel
    in the frames' own order, or ValueError."""
    if isinstance(colour, int) and not isinstance(colour, bool):
        if 0 <= colour < (1 << 24):
            return colour
    else:
        try:
            c = [int(v) for v in colour]
            if len(c) == 3 and all(0 <= v <= 255 and v == w for v, w in zip(c, colour)):
                return c[0] | (c[1] << 8) | (c[2] << 16)
        except (TypeError, ValueError):
            pass
    raise ValueError('%s: colour = %r: a number below 2^24, or the three bytes of a pixel, 0..255 each' % (what, colour))


def _checked(what, kind, W, H, softness, colour):
    try:
        kind = kind_of(kind, what)
        colour = colour_of(colour, what)
    except ValueError as e:
        raise _native.KbeError(str(e)) from None
    if softness is None:
        softness = default_softness(kind, W, H)
    if not (isinstance(softness, int) and not isinstance(softness, bool) and 1 <= softness <= MAX_SOFTNESS):
        raise _native.KbeError('%s: softness = %r: 1..%d' % (what, softness, MAX_SOFTNESS))
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise _native.KbeError('%s: frames of %d x %d: 1..%d either way' % (what, W, H, MAX_SIDE))
    return kind, softness, colour


def _frames(f, what, name):
    import torch
    if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 4 and f.size(3) == 3 and f.size(0) >= 1 and f.is_contiguous()):
        raise _native.KbeError('%s takes contiguous uint8 [n,H,W,3] tensors on the GPU (%s: %s)' % (
            what, name, '%s %s on %s' % (tuple(f.shape), f.dtype, f.device) if torch.is_tensor(f) else type(f).__name__))
    return f


def _enqueue(sources, others, n, W, H, kind, progress, softness, colour, targets):
    """The module's one call of the entry: tables of n frame addresses, rows of 3 W bytes, on the current stream."""
    table = (ctypes.c_int32 * n)(*progress)
    _call('kbe_transition_u8', sources, others, n, W, H, 3 * W, kind, table, softness, colour, targets, 3 * W, _native._stream())


def blend(frames_from, frames_to, kind, progress, softness=None, colour=0, out=None):
    """Two uint8 [n,H,W,3] tensors in HBM of one shape -> a new uint8 [n,H,W,3] tensor on the same device (or `out`, filled), frame i made of
    frames_from[i] and frames_to[i] at progress[i] in 0..256; kind: a name of KINDS or its number; softness: the wipes' edge in pixels
    (default_softness); colour: the fade's (colour_of).  Asynchronous on the current stream."""
    import torch
    what = 'transition.blend'
    a, b = _frames(frames_from, what, 'frames_from'), _frames(frames_to, what, 'frames_to')
    if a.shape != b.shape or a.device != b.device:
        raise _native.KbeError('%s: frames_from is %s on %s and frames_to %s on %s: one shape, one device' % (what, tuple(a.shape), a.device, tuple(b.shape), b.device))
    n, H, W, _, sources = _native.frame_pointers(a, what)
    others = _native.frame_pointers(b, what)[4]
    kind, softness, colour = _checked(what, kind, W, H, softness, colour)
    try:
        progress = [int(p) for p in progress]
    except (TypeError, ValueError):
        progress = None
    if progress is None or len(progress) != n or not all(0 <= p <= 256 for p in progress):
        raise _native.KbeError('%s: progress: %d values 0..256, one per frame' % (what, n))
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=a.device)
    elif _frames(out, what, 'out').shape != a.shape or out.device != a.device:
        raise _native.KbeError('%s: out is %s on %s: the shape and the device of the frames, %s on %s' % (what, tuple(out.shape), out.device, tuple(a.shape), a.device))
    targets = _native.frame_pointers(out, what)[4]
    _enqueue(sources, others, n, W, H, kind, progress, softness, colour, targets)
    return out


def join_plan(lengths, T, fade_in=0, fade_out=0):
    """Where every frame of a slideshow comes from: for clips of `lengths` frames joined by transitions of T frames, a list with one item per
    output frame, sum(lengths) - (k - 1) T of them:
        ('clip', i, j)                           frame j of clip i as it is;
        ('junction', i, i + 1, j, j2, p)         made of frame j of clip i and frame j2 of clip i + 1 at the progress p of progress_table(T);
        ('fade-in', i, j, p), ('fade-out', i, j, p)   frame j of clip i faded from / to the colour: FADE(frame, frame, p).
    The T frames of a junction are the last T of clip i and the first T of clip i + 1; 1 <= T <= min(lengths) // 2 with two clips or more.
    fade_in, fade_out: the show's first / last frames; they must lie in the part of the first / last clip that no junction uses.  ValueError otherwise."""
    lengths = [int(v) for v in lengths]
    k, fade_in, fade_out = len(lengths), int(fade_in), int(fade_out)
    if k < 1 or min(lengths) < 1:
        raise ValueError('transition.join: %r: one clip or more, of one frame or more each' % (lengths,))
    T = int(T) if k > 1 else 0
    if k > 1 and not 1 <= T <= min(lengths) // 2:
        raise ValueError('transition.join: T = %d: 1..%d, half of the shortest clip (%d frames)' % (T, min(lengths) // 2, min(lengths)))
    free_first, free_last = lengths[0] - T, lengths[-1] - T
    if not 0 <= fade_in <= free_first:
        raise ValueError('transition.join: fade_in = %d: 0..%d, the frames of the first clip that no junction uses' % (fade_in, free_first))
    if not 0 <= fade_out <= free_last:
        raise ValueError('transition.join: fade_out = %d: 0..%d, the frames of the last clip that no junction uses' % (fade_out, free_last))
    if k == 1 and fade_in + fade_out > lengths[0]:
        raise ValueError('transition.join: fade_in + fade_out = %d: at most the clip\'s %d frames' % (fade_in + fade_out, lengths[0]))
    table = progress_table(T)
    plan = []
    for i, n in enumerate(lengths):
        plan += [('clip', i, j) for j in range(T if i > 0 else 0, n - T if i + 1 < k else n)]
        if i + 1 < k:
            plan += [('junction', i, i + 1, n - T + j, j, table[j]) for j in range(T)]
    for j, p in enumerate(progress_table(fade_in)):
        plan[j] = ('fade-in', 0, plan[j][2], 128 + p // 2)
    for j, p in enumerate(progress_table(fade_out)):
        at = len(plan) - fade_out + j
        plan[at] = ('fade-out', k - 1, plan[at][2], p // 2)
    return plan


def join(clips, kind, T, softness=None, colour=0, fade_in=0, fade_out=0):
    """A list of k >= 1 clips, uint8 [n_i,H,W,3] tensors in HBM of one H x W -> ONE new tensor of sum(n_i) - (k - 1) T frames (join_plan): the
    clips' bodies copied on the device, the T frames of every junction and the faded frames written straight into their place by the entry,
    from the clips' own frames.  Asynchronous on the current stream."""
    import torch
    what = 'transition.join'
    clips = [_frames(c, what, 'clip %d' % i) for i, c in enumerate(clips)]
    if not clips:
        raise _native.KbeError('%s: no clip' % what)
    H, W = int(clips[0].shape[1]), int(clips[0].shape[2])
    for i, c in enumerate(clips):
        if tuple(c.shape[1:3]) != (H, W) or c.device != clips[0].device:
            raise _native.KbeError('%s: clip %d is %d x %d on %s and clip 0 is %d x %d on %s: one size, one device' % (what, i, c.shape[2], c.shape[1], c.device, W, H, clips[0].device))
    kind, softness, colour = _checked(what, kind, W, H, softness, colour)
    try:
        plan = join_plan([c.shape[0] for c in clips], T, fade_in, fade_out)
    except ValueError as e:
        raise _native.KbeError(str(e)) from None
    out = torch.empty((len(plan), H, W, 3), dtype=torch.uint8, device=clips[0].device)
    step = 3 * W * H
    bases = [_native.frame_pointers(c, what)[4] for c in clips]
    base = _native.frame_pointers(out, what)[4][0]
    # runs of the plan: a clip's frames in a row are one copy, a junction's or a fade's frames one call
    at = 0
    while at < len(plan):
        end = at + 1
        while end < len(plan) and plan[end][:2] == plan[at][:2]:
            end += 1
        item, n = plan[at], end - at
        if item[0] == 'clip':
            out[at:end].copy_(clips[item[1]][item[2]:item[2] + n])
        else:
            junction = item[0] == 'junction'
            sources = (ctypes.c_void_p * n)(*[bases[q[1]][q[3 if junction else 2]] for q in plan[at:end]])
            others = (ctypes.c_void_p * n)(*[bases[q[2]][q[4]] for q in plan[at:end]]) if junction else sources
            targets = (ctypes.c_void_p * n)(*[base + (at + j) * step for j in range(n)])
            _enqueue(sources, others, n, W, H, kind if junction else FADE, [q[-1] for q in plan[at:end]], softness, colour, targets)
        at = end
    return out
