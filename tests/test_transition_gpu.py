"""The transitions on the GPU (include/kbe_transition.h; kernel: csrc/kbe_transition.hip): kbe_transition_u8 byte for byte against the NumPy twin
(tests/transition_cases.py) under guard bands and both poisons, at the shapes where the kernel can go wrong -- rows shorter than a piece, rows
around a workgroup's span, a soft edge across a span's end, every combination of alignment classes, the cut into launches, the lanes that
read one source only --, every refusal, a side stream, and the host side built on it (transition.blend, transition.join, Pipeline.render,
slideshow.make)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import encoder_gpu as eg
import gif_cases as gc
import stream_gpu
import transition_cases as tc
import transition_gpu as tg

pytestmark = pytest.mark.gpu
run, assert_blend = tg.run_transition, tg.assert_blend
KINDS = sorted(tc.KINDS)


@pytest.fixture(scope='module')
def TR():
    from ken_burns_effect_amd import transition
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    transition.load()
    return transition


# -- the entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('frame', tc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(TR, frame, kind):
    """37x50, 64x48 and 160x128 frames, every kind; two frames in one call at p = 128 and 85; output rows padded by 4.  (That the inputs
    tell -- the dissolve differs from both sources, the wipes' weights hold 0, 256 and what lies between, the fade's colour bytes are not
    interchangeable -- is asserted on the same frames in tests/test_transition_stream.py.)"""
    W, H = frame
    a, b = tc.frames_of(W, H)
    want = tc.twin_of(W, H, kind)
    assert not np.array_equal(want, a) and not np.array_equal(want, b) and not np.array_equal(want[0], want[1])
    assert_blend(TR, a, b, kind, tc.PROGRESS, want, tc.SOFTNESS, tc.COLOUR, out_pad=4)


@pytest.mark.parametrize('frame', [(1, 7), (2, 7), (5, 7), (16, 7), (1366, 3)], ids=lambda v: '%dx%d' % v)
def test_narrow_and_awkward_rows(TR, frame):
    """W = 1, 2 and 5: a row shorter than one 16-byte piece, which an unaligned row still cuts in two.  W = 16: exactly three pieces.
    1366 x 3: rows of 4098 bytes, two bytes beyond four spans.  Aligned, and 13 bytes off with `from` 7 and `to` 2 bytes off, source rows 3 bytes apart."""
    W, H = frame
    a, b = tc.frames_of(W, H)
    for kind in KINDS:
        want = tc.twin_blend(a, b, kind, (77, 200), 3, tc.COLOUR)
        assert_blend(TR, a, b, kind, (77, 200), want, 3, tc.COLOUR)
        assert_blend(TR, a, b, kind, (77, 200), want, 3, tc.COLOUR, pad=3, out_pad=1, shift=13, src_shift=7, to_shift=2)


@pytest.mark.parametrize('end', [tg.SPAN - 1, tg.SPAN, tg.SPAN + 1])
def test_rows_around_a_workgroups_span(TR, end):
    """A workgroup takes SPAN = 1024 bytes of a row, counted from the row's address rounded down to 16.  Rows of 341 pixels, 1023 bytes, at an
    output stride of 1024: moved 0, 1 and 2 bytes off the allocation every row ends one byte short of the span, exactly on it, and one byte
    beyond it, in a second workgroup whose only piece is one byte.  5 rows: a second workgroup down the frame as well."""
    W, H = 341, 5
    assert tg.SPAN == 1024 and 3 * W == tg.SPAN - 1
    a, b = tc.frames_of(W, H, 1)
    for kind, p in (('dissolve', 128), ('wipe-left', 20), ('wipe-right', 250), ('wipe-up', 128), ('fade', 200)):
        want = tc.twin_blend(a, b, kind, [p], 40, tc.COLOUR)
        assert (want[:, :, -1] != a[:, :, -1]).any() and (want[:, :, -1] != b[:, :, -1]).any()           # the row's last pixel is blended
        assert_blend(TR, a, b, kind, [p], want, 40, tc.COLOUR, out_pad=1, shift=end - 3 * W, to_shift=3, aligned=True)


@pytest.mark.parametrize('kind,p', [('wipe-right', 210), ('wipe-left', 45)])
def test_a_soft_edge_across_a_spans_end(TR, kind, p):
    """W = 400, s = 40, the output aligned: byte 1024 of a row begins the second workgroup's span, and the soft edge lies on both sides of it."""
    W, H, s = 400, 6, 40
    soft = tc.soft_edge(kind, p, W, H, s).reshape(H, 3 * W)
    assert soft[:, tg.SPAN - 48:tg.SPAN + 48].all() and not soft[:, :tg.SPAN - 128].any() and not soft[:, tg.SPAN + 128:].any()
    values = np.unique(tc.weight_map(kind, p, W, H, s))
    assert values[0] == 0 and values[-1] == 256 and len(values) >= s - 1
    a, b = tc.frames_of(W, H, 1)
    assert_blend(TR, a, b, kind, [p], None, s, 0, aligned=True)
    assert_blend(TR, a, b, kind, [p], None, s, 0, shift=5, src_shift=1, to_shift=2, pad=1)


@pytest.mark.parametrize('shift', range(16))
def test_every_combination_of_alignment_classes(TR, shift):
    """37 x 17 frames, source rows at a stride of 117 and output rows at one of 113, so that a frame's rows walk through all classes: a
    source's modulo 4 -- what a lane's funnel shift depends on --, the output's modulo 16.  The entry has ONE stride for both sources, so
    `to` gets classes of its own by its own offset: the output moved `shift` bytes off its allocation and `to` shift / 4 bytes.  The sixteen
    calls reach all 256 combinations of (from class, to class, output class)."""
    W, H = 37, 17
    triples = {((117 * y) % 4, (s // 4 + 117 * y) % 4, (s + 113 * y) % 16) for s in range(16) for y in range(H)}
    assert len(triples) == 4 * 4 * 16
    a, b = tc.frames_of(W, H, 1)
    for kind, p in (('dissolve', 128), ('wipe-right', 150), ('wipe-left', 90), ('fade', 60), ('fade', 190)):
        assert_blend(TR, a, b, kind, [p], None, 9, tc.COLOUR, pad=6, out_pad=2, shift=shift, to_shift=shift // 4, aligned=True)


def test_the_extremes(TR):
    """All-255 against all-0 at p = 1, 128 and 255; softness 1 and 3 W; p = 0 and 256 equal to the sources where they lie, for every kind."""
    W, H = 37, 9
    white, black = np.full((3, H, W, 3), 255, np.uint8), np.zeros((3, H, W, 3), np.uint8)
    a, b = tc.frames_of(W, H, 2)
    for kind in KINDS:
        for s in (1, 3 * W):
            assert_blend(TR, white, black, kind, (1, 128, 255), None, s, 0xFFFFFF)
            assert_blend(TR, black, white, kind, (1, 128, 255), None, s, 0)
            assert_blend(TR, a, b, kind, (0, 256), np.stack([a[0], b[1]]), s, tc.COLOUR, pad=2, src_shift=1, to_shift=6, shift=3)
    assert (tc.twin_blend(white, black, 'dissolve', (1, 128, 255)) == np.array([254, 128, 1], np.uint8)[:, None, None, None]).all()


def test_from_and_to_are_the_same_frames(TR):
    """The two tables hold the same pointers: the frame itself under the dissolve and every wipe, the twin of (a, a) under the fade."""
    W, H = 37, 20
    a, b = tc.frames_of(W, H, 2)
    for kind in KINDS:
        want = tc.twin_blend(a, a, kind, (77, 200), 5, tc.COLOUR)
        assert (kind == 'fade') != np.array_equal(want, a)
        assert_blend(TR, a, b, kind, (77, 200), want, 5, tc.COLOUR, same=True, pad=1)


@pytest.mark.parametrize('kind', ['dissolve', 'wipe-down', 'fade'])
def test_the_cut_into_launches(TR, kind):
    """A launch carries 12 frames: 13 frames with 13 values of p are 12 + 1, every output another."""
    W, H, n = 21, 6, 13
    a, b = tc.frames_of(W, H, n)
    progress = [3 + 19 * i for i in range(n)]
    want = tc.twin_blend(a, b, kind, progress, 2, tc.COLOUR)
    assert len({want[i].tobytes() for i in range(n)}) == n and len(set(progress)) == n and TR.FRAMES_PER_LAUNCH == 12
    swapped = tc.twin_blend(a, b, kind, progress[1:] + progress[:1], 2, tc.COLOUR)
    assert all(not np.array_equal(swapped[i], want[i]) for i in range(n))                   # (a frame at another frame's progress shows)
    assert_blend(TR, a, b, kind, progress, want, 2, tc.COLOUR)


@pytest.mark.parametrize('kind,p', [('wipe-right', 100), ('wipe-left', 100), ('wipe-down', 100), ('wipe-up', 100), ('fade', 100), ('fade', 180), ('dissolve', 0), ('dissolve', 256)])
def test_a_source_that_is_not_needed_is_not_looked_at(TR, kind, p):
    """A wipe with s = 1: outside its edge a byte is a copy of one source.  In a second run every byte of `from` whose weight is 256 and every
    byte of `to` whose weight is 0 holds another picture: the output does not change.  The fade reads one source, the dissolve at its ends too.
    What this holds the kernel to is that those bytes have no influence -- a wrong weight at the edge's border, or a lane that mixed its
    sources up, shows.  It cannot show that the load itself is skipped: blend(a, b, 0) = a whatever b is, so a kernel that loaded both sources
    would pass as well.  That the load is skipped is in the source (the plan's `from` / `to` in front of load_piece, csrc/kbe_transition.hip)
    and in the time: the vertical wipes and the fade take about three quarters of the dissolve's (tools/transition_time.py)."""
    W, H = 160, 12
    a, b = tc.frames_of(W, H, 1)
    other = gc.photo_like(H, W, 99)[None]
    if kind == 'fade':
        from_unread, to_unread = np.full(a.shape, p > 128), np.full(a.shape, p <= 128)
    else:
        w = np.broadcast_to(tc.weight_map(kind, p, W, H, 1)[None, :, :, None], a.shape)
        from_unread, to_unread = w == 256, w == 0
        assert not ((w > 0) & (w < 256)).any() or kind.startswith('wipe')
        assert from_unread.any() or to_unread.any()
    assert (other != a).mean() > 0.5 and (other != b).mean() > 0.5
    want = tc.twin_blend(a, b, kind, [p], 1, tc.COLOUR)
    for poison in tg.POISONS:
        for first, second in ((a, b), (np.where(from_unread, other, a), np.where(to_unread, other, b))):
            rc, got = run(TR, first, second, kind, [p], 1, tc.COLOUR, poison=poison, src_shift=3)
            assert rc == 0 and np.array_equal(got.reshape(1, H, W, 3), want)


def _out_bytes(a):
    return (a['H'] - 1) * a['out_stride_bytes'] + 3 * a['W']


OVERLAPS_SOURCE, OVERLAPS_OUTPUT = 'an element of out_u8 overlaps a source frame', 'an element of out_u8 overlaps another output'
REFUSALS = {'null from': (lambda a: a.update(from_u8=None), 'null from_u8'), 'null to': (lambda a: a.update(to_u8=None), 'null to_u8'),
            'null outputs': (lambda a: a.update(out_u8=None), 'null out_u8'), 'null progress': (lambda a: a.update(progress=None), 'null progress'),
            'n = 0': (lambda a: a.update(n=0), 'n < 1'),
            'W = 65536': (lambda a: a.update(W=65536, stride_bytes=3 * 65536, out_stride_bytes=3 * 65536), 'W or H outside 1..65535'),
            'H = 0': (lambda a: a.update(H=0), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'out stride < 3 W': (lambda a: a.update(out_stride_bytes=3 * a['W'] - 1), 'out_stride_bytes < 3 W'),
            'kind 6': (lambda a: a.update(kind=6), 'kind outside 0..5'), 'kind -1': (lambda a: a.update(kind=-1), 'kind outside 0..5'),
            'progress 257': (lambda a: a['progress'].__setitem__(1, 257), 'an element of progress outside 0..256'),
            'progress -1': (lambda a: a['progress'].__setitem__(0, -1), 'an element of progress outside 0..256'),
            'softness 0': (lambda a: a.update(softness=0), 'softness outside 1..65535'), 'softness 65536': (lambda a: a.update(softness=65536), 'softness outside 1..65535'),
            'colour bit 24': (lambda a: a.update(colour=1 << 24), 'colour with bits 24..31 set'),
            'null from 1': (lambda a: a['from_u8'].__setitem__(1, None), 'null element of from_u8'), 'null to 0': (lambda a: a['to_u8'].__setitem__(0, None), 'null element of to_u8'),
            'null output 1': (lambda a: a['out_u8'].__setitem__(1, None), 'null element of out_u8'),
            'output is a from frame': (lambda a: a['out_u8'].__setitem__(1, a['from_u8'][1]), OVERLAPS_SOURCE),
            'output is the other outputs to frame': (lambda a: a['out_u8'].__setitem__(0, a['to_u8'][1]), OVERLAPS_SOURCE),
            # (the frames lie a gap apart: the output ends on the first byte of the next source and touches no other)
            'one byte of the next from frame': (lambda a: a['out_u8'].__setitem__(0, a['from_u8'][1] - _out_bytes(a) + 1), OVERLAPS_SOURCE),
            'one byte of the next to frame': (lambda a: a['out_u8'].__setitem__(1, a['to_u8'][1] - _out_bytes(a) + 1), OVERLAPS_SOURCE),
            'one byte of the other output': (lambda a: a['out_u8'].__setitem__(0, a['out_u8'][1] - _out_bytes(a) + 1), OVERLAPS_OUTPUT),
            'the same output twice': (lambda a: a['out_u8'].__setitem__(0, a['out_u8'][1]), OVERLAPS_OUTPUT)}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(TR, what):
    from ken_burns_effect_amd import _native
    W, H = tc.FRAMES[0]
    change, text = REFUSALS[what]
    a, b = tc.frames_of(W, H)
    rc, got = run(TR, a, b, 'wipe-right', tc.PROGRESS, gap=3 * W * H + 64, change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_transition_u8: ' + text
    assert (got == 0xFF).all()


def _pointers(t):
    return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])


def test_on_a_side_stream_behind_a_delay(TR):
    """The entry called raw with the handle of a non-blocking side stream behind stream_gpu's delay: it returns while the delay runs, and the
    result is the twin, bit for bit; the sources hold a decoy until the delay has run out."""
    from ken_burns_effect_amd import _native
    n, H, W = 13, 37, 50
    right = [torch.from_numpy(f).cuda() for f in tc.frames_of(W, H, n)]
    decoy = [torch.from_numpy(f).cuda() for f in tc.frames_of(W, H, n, 150)]
    frames, out = [t.clone() for t in decoy], torch.zeros(n, H, W, 3, dtype=torch.uint8, device='cuda')
    progress = [10 + 18 * i for i in range(n)]

    def call():
        TR._call('kbe_transition_u8', _pointers(frames[0]), _pointers(frames[1]), n, W, H, 3 * W, TR.KINDS['wipe-right'], (ctypes.c_int32 * n)(*progress), 6, 0,
                 _pointers(out), 3 * W, _native._stream())
        return out
    what = 'transition_u8'
    got, want = stream_gpu.hold(what, 'bits', frames, right, decoy, call, written=lambda: [out])
    assert what in stream_gpu.ENQUEUED                                      # (the entry had returned while the delay still ran)
    assert np.array_equal(got[0], tc.twin_blend(right[0].cpu().numpy(), right[1].cpu().numpy(), 'wipe-right', progress, 6)) and np.array_equal(got[0], want[0])


# -- the module ----------------------------------------------------------------------------------
def test_blend_and_its_refusals(TR):
    from ken_burns_effect_amd import _native
    W, H = tc.FRAMES[2]
    n = 13
    a, b = tc.frames_of(W, H, n)
    fa, fb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    progress = TR.progress_table(n)
    got = TR.blend(fa, fb, 'wipe-left', progress)
    assert got.shape == (n, H, W, 3) and got.dtype == torch.uint8 and got.device == fa.device
    assert TR.default_softness('wipe-left', W, H) == 20 and np.array_equal(got.cpu().numpy(), tc.twin_blend(a, b, 'wipe-left', progress, 20))
    assert np.array_equal(TR.blend(fa, fb, 5, progress, colour=(10, 200, 90)).cpu().numpy(), tc.twin_blend(a, b, 'fade', progress, 1, tc.COLOUR))
    out = torch.zeros_like(fa)
    assert TR.blend(fa, fb, 'wipe-down', progress, softness=3, out=out) is out and np.array_equal(out.cpu().numpy(), tc.twin_blend(a, b, 'wipe-down', progress, 3))
    assert torch.equal(TR.blend(fa, fb, 'dissolve', [0] * n), fa) and torch.equal(TR.blend(fa, fb, 'dissolve', [256] * n), fb) and torch.equal(TR.blend(fa, fa, 'wipe-up', progress), fa)
    for args, kw in (((fa.cpu(), fb, 0, progress), {}), ((fa, fb.int(), 0, progress), {}), ((fa, fb[:, :, ::2], 0, progress), {}), ((fa[0], fb[0], 0, progress), {}),
                     ((fa, fb[:12], 0, progress), {}), ((fa, fb, 'iris', progress), {}), ((fa, fb, 6, progress), {}), ((fa, fb, 0, progress[:12]), {}),
                     ((fa, fb, 0, [257] * n), {}), ((fa, fb, 0, None), {}), ((fa, fb, 1, progress), dict(softness=0)), ((fa, fb, 1, progress), dict(softness=65536)),
                     ((fa, fb, 5, progress), dict(colour=1 << 24)), ((fa, fb, 5, progress), dict(colour=(1, 2))), ((fa, fb, 0, progress), dict(out=out[:12])),
                     ((fa, fb, 0, progress), dict(out=out.cpu())), ((fa, fb, 0, progress), dict(out=fa))):
        with pytest.raises(_native.KbeError, match=r'transition\.blend|kbe_transition_u8: an element of out_u8 overlaps a source frame'):
            TR.blend(*args, **kw)


@pytest.fixture(scope='module')
def clips():
    """Two clips of smoke()'s 128 x 96 scene with different seeds, 6 steps each, left in HBM."""
    from ken_burns_effect_amd import common, synthetic
    K = eg.kernels()
    H, W = 96, 128
    made = []
    for seed in (0, 1):
        image, disp = synthetic.make_rgbd(H, W, seed=seed)
        depth = (synthetic.FOCAL * synthetic.BASELINE) / (disp + 1e-7)
        oc = {'dblFocal': synthetic.FOCAL, 'dblBaseline': synthetic.BASELINE, 'intWidth': W, 'intHeight': H, 'objectDepthrange': synthetic.depthrange_of(depth),
              'tensorRawImage': image.cuda(), 'tensorRawDisparity': disp.cuda(), 'tensorRawDepth': depth.cuda()}
        oc['tensorRawPoints'] = K.depth_to_points(oc['tensorRawDepth'], synthetic.FOCAL).view(1, 3, -1)
        ofrom, oto = synthetic.default_windows(H, W)
        settings = {'dblSteps': np.linspace(0.0, 1.0, 6).tolist(), 'objectFrom': ofrom, 'objectTo': oto, 'boolInpaint': False, 'dolly': False}
        common._reset_inpa(oc)
        made.append(common.render_frames(common.frame_cameras(settings, oc), oc, common.crop_size(settings), keep_on_device=True).clone())
    assert made[0].shape == made[1].shape and made[0].shape[0] == 6 and made[0].is_cuda and not torch.equal(made[0], made[1])
    return made


def test_join_on_rendered_clips(TR, clips):
    """T = 2: the bodies are the clips' frames, the junction's frames the twin of the named pairs, the fades the twin; the clips are only read."""
    from ken_burns_effect_amd import _native
    host = [c.cpu().numpy() for c in clips]
    colour = (10, 200, 90)
    for kind in ('dissolve', 'wipe-right', 'fade'):
        got = TR.join(clips, kind, 2, 7, colour, fade_in=2, fade_out=3)
        plan = TR.join_plan([6, 6], 2, 2, 3)
        assert got.shape == (10,) + clips[0].shape[1:] and got.is_cuda and len(plan) == 10
        assert [q[0] for q in plan] == ['fade-in'] * 2 + ['clip'] * 2 + ['junction'] * 2 + ['clip'] + ['fade-out'] * 3
        got = got.cpu().numpy()
        for i, item in enumerate(plan):
            if item[0] == 'clip':
                want = host[item[1]][item[2]]
            elif item[0] == 'junction':
                want = tc.twin_blend(host[item[1]][item[3]][None], host[item[2]][item[4]][None], kind, [item[5]], 7, tc.COLOUR)[0]
                assert not any(np.array_equal(want, f) for c in host for f in c)
            else:
                frame = host[item[1]][item[2]][None]
                want = tc.twin_blend(frame, frame, 'fade', [item[3]], 7, tc.COLOUR)[0]
                assert not np.array_equal(want, frame[0])
            assert np.array_equal(got[i], want), (kind, i, item)
    assert all(np.array_equal(c.cpu().numpy(), h) for c, h in zip(clips, host))
    assert torch.equal(TR.join(clips[:1], 'dissolve', 99), clips[0]) and TR.join(clips[:1], 'dissolve', 1).data_ptr() != clips[0].data_ptr()
    three = TR.join([clips[0], clips[1][:4], clips[0]], 'wipe-up', 2)
    assert three.shape[0] == 12 and torch.equal(three[:4], clips[0][:4]) and torch.equal(three[8:], clips[0][2:])
    for bad, T, kw in ((clips, 4, {}), (clips, 0, {}), (clips, 2, dict(fade_in=5)), ([clips[0], clips[1][:, :48]], 2, {}), (clips, 2, dict(softness=0)), (clips, 2, dict(colour=(1, 2, 300)))):
        with pytest.raises(_native.KbeError, match=r'transition\.join'):
            TR.join(bad, 'dissolve', T, **kw)


# -- the route ---------------------------------------------------------------------------------
ENV = ('KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER', 'KBE_SHUTTER_SAMPLES', 'KBE_Y4M')


def _files(directory):
    return {str(p.relative_to(directory)): p.read_bytes() for p in sorted(directory.rglob('*')) if p.is_file()}


class OneRenderPerClip:
    """common.process_kenburns as the pipeline module sees it, with a memory: the first call for a photo (the bytes of objectCommon's image), a
    camera path, an output size, a lens and a shutter renders -- once, into HBM --, and every later call with the same arguments gets those
    frames again, as a device tensor or as the list of host arrays by ``keep_on_device``.  Two renders of one photo need not agree to the
    byte (the networks run again in every call, and theirs is not a bit-exact route), so what a test wants to know of two calls -- that they
    ask for the same frames and treat them alike afterwards -- is asked on ONE set of frames: a call that passes other settings, another
    size or another photo misses the memory, renders for itself, and shows in ``rendered``."""

    def __init__(self, real):
        self.real, self.kept, self.rendered, self.calls = real, {}, [], []

    def __call__(self, settings, oc, module, keep_on_device=False, **kw):
        key = (oc['tensorRawImage'].cpu().numpy().tobytes(), repr(sorted((k, repr(v)) for k, v in settings.items())), repr(sorted((k, repr(v)) for k, v in kw.items())))
        self.calls.append(key)
        if key not in self.kept:
            self.kept[key] = self.real(settings, oc, module, keep_on_device=True, **kw).clone()
            self.rendered.append(key)
        frames = self.kept[key]
        if keep_on_device:
            return frames.clone()
        host = frames.cpu().numpy()
        return [host[i] for i in range(host.shape[0])]


def test_render_and_a_slideshow(TR, tmp_path, monkeypatch):
    """One Pipeline (seeded weights, 6 steps, --write-frames) and two synthetic 64 x 48 photos, every clip rendered once (OneRenderPerClip).
    Pipeline.render asks for the frames Pipeline.__call__ asks for and returns them, with and without a width; slideshow.make with T = 2,
    --gif and --y4m writes slideshow.mp4, slideshow.gif (10 frames), slideshow.y4m (10 FRAMEs) and frames/0..9.png, which decode to the
    frames returned; its bodies are the clips' frames, frames 4 and 5 the twin of the named pairs and no frame of either clip; one photo
    and no fades give Pipeline.render's frames; and a Pipeline call writes the same bytes before and after."""
    from ken_burns_effect_amd import kbe, pipeline, slideshow, synthetic, yuv
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    images = [synthetic.make_rgbd(48, 64, seed)[0] for seed in (12, 13)]
    zoom = kbe.windows_for(64, 48, slideshow.NO_WINDOW, False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=6)
    once = OneRenderPerClip(pipeline.common.process_kenburns)
    monkeypatch.setattr(pipeline.common, 'process_kenburns', once)
    before = pipe(images[0], zoom, str(tmp_path / 'before'))
    assert len(once.rendered) == 1
    rendered = []
    for image in images:
        frames = pipe.render(image, zoom)
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.shape == (6, 48, 64, 3)
        rendered.append(frames.cpu().numpy())
    # (render asked for the first photo's frames with __call__'s own arguments: nothing was rendered for it, and it returns what __call__ returned)
    assert len(once.rendered) == 2 and once.calls[1] == once.calls[0] and once.calls[2] != once.calls[0]
    assert np.array_equal(rendered[0], np.stack(before)) and not np.array_equal(rendered[0], rendered[1])
    pipe.width = 32
    narrow = pipe.render(images[0], zoom)
    assert len(once.rendered) == 3 and 'out_size' in once.calls[-1][2] and '(32, 24)' in once.calls[-1][2]
    assert narrow.shape == (6, 24, 32, 3) and np.array_equal(narrow.cpu().numpy(), np.stack(pipe(images[0], zoom, None))) and once.calls[-1] == once.calls[-2]
    pipe.width = None

    got = slideshow.make(images, str(tmp_path / 'show'), pipe, 'dissolve', 2, gif=True, y4m=True)
    assert len(once.rendered) == 3 and once.calls[-2:] == [once.calls[0], once.calls[2]]            # (make's two clips are render's, by render's arguments)
    files = _files(tmp_path / 'show')
    assert sorted(files) == sorted(['slideshow.mp4', 'slideshow.gif', 'slideshow.y4m'] + ['frames/%d.png' % i for i in range(10)])
    assert len(got) == 10 and all(f.shape == (48, 64, 3) and f.dtype == np.uint8 for f in got)
    gif = Image.open(str(tmp_path / 'show' / 'slideshow.gif'))
    assert gif.size == (64, 48) and gif.n_frames == 10
    header = yuv.y4m_header(64, 48, 25)
    assert files['slideshow.y4m'].startswith(header + b'FRAME\n') and len(files['slideshow.y4m']) == len(header) + 10 * (6 + yuv.frame_bytes(64, 48))
    for i, frame in enumerate(got):
        png = Image.open(str(tmp_path / 'show' / 'frames' / ('%d.png' % i)))
        assert png.size == (64, 48) and np.array_equal(np.asarray(png.convert('RGB')), frame[:, :, ::-1])
    table = TR.progress_table(2)
    for i in range(10):
        if i in (4, 5):
            want = tc.twin_blend(rendered[0][i][None], rendered[1][i - 4][None], 'dissolve', [table[i - 4]])[0]
            assert not any(np.array_equal(got[i], f) for clip in rendered for f in clip)
        else:
            want = rendered[0][i] if i < 4 else rendered[1][i - 4]
        assert np.array_equal(got[i], want), i
    # one photo and no fades: the frames of Pipeline.render byte for byte, and nothing written without a directory
    assert np.array_equal(np.stack(slideshow.make(images[1:], None, pipe, 'wipe-left', 99)), rendered[1]) and once.calls[-1] == once.calls[2]
    with pytest.raises(ValueError, match=r'^--transition-frames 4: 1\.\.3'):
        slideshow.make(images, str(tmp_path / 'refused'), pipe, 'dissolve', 4)
    assert not (tmp_path / 'refused').exists() and len(once.rendered) == 3

    pipe(images[0], zoom, str(tmp_path / 'after'))
    assert once.calls[-1] == once.calls[0] and len(once.rendered) == 3
    assert _files(tmp_path / 'after') == _files(tmp_path / 'before') and sorted(_files(tmp_path / 'before')) == ['3d_kbe.mp4'] + ['frames/%d.png' % i for i in range(6)]
