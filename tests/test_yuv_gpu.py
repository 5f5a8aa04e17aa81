"""The 4:2:0 planes on the GPU (include/kbe_yuv.h; kernel: csrc/kbe_yuv.hip): kbe_yuv420_u8 byte for byte against the NumPy twin
(tests/yuv_cases.py) under guard bands and both poisons, at the shapes where the kernel can go wrong -- frames narrower than a lane's run, odd
widths and heights, row pairs around a wave's span, every pair of alignment classes, the cut into launches, the widest and the tallest frame --,
every refusal, a side stream, and the host side built on it (yuv.convert, yuv.planes, yuv.write_y4m, Pipeline(y4m=True))."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import stream_gpu
import yuv_cases as yc
import yuv_gpu as yg

pytestmark = pytest.mark.gpu
run, assert_planes = yg.run_yuv, yg.assert_planes


@pytest.fixture(scope='module')
def YUV():
    from ken_burns_effect_amd import yuv
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    yuv.load()
    return yuv


# -- the entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize('bgr', [False, True], ids=['rgb', 'bgr'])
@pytest.mark.parametrize('frame', yc.FRAMES, ids=lambda v: '%dx%d' % v)
def test_the_device_is_the_twin_byte_for_byte(YUV, frame, bgr):
    """37x50, 64x48 and 160x128 frames, two a call, both flag values, source rows padded by 5 -- on frames where a copied channel, one chroma
    plane for the other or the wrong channel order differ from the right planes in more than 0.9 of their bytes."""
    W, H = frame
    frames = yc.frames_of(W, H)
    yc.assert_telling(frames)
    assert_planes(YUV, frames, yc.twin_of(W, H, bgr), bgr=bgr, pad=5)


@pytest.mark.parametrize('frame', [(1, 1), (1, 2), (2, 1), (3, 3), (5, 7), (16, 2), (17, 3), (yg.SPAN + 2, 2)], ids=lambda v: '%dx%d' % v)
def test_narrow_and_awkward_frames(YUV, frame):
    """Frames of one pixel, one column, one row; cells of one and two pixels; exactly one run and one pixel more; and a row pair of 1026 pixels,
    two beyond a wave's span: a second trip whose only lane has two pixels.  Aligned, and with the source 7 and the payload 13 bytes off."""
    W, H = frame
    frames = yc.frames_of(W, H, 3, 9)
    for bgr in (False, True):
        assert_planes(YUV, frames, bgr=bgr)
        assert_planes(YUV, frames, bgr=bgr, pad=3, shift=13, src_shift=7)


@pytest.mark.parametrize('W', [yg.SPAN - 1, yg.SPAN, yg.SPAN + 1])
def test_rows_around_a_waves_span(YUV, W):
    """A wave takes SPAN = 1024 pixels of a row pair in one trip.  Rows that end one pixel -- one byte of Y -- short of it, exactly on it, and
    one beyond it, in a second trip; 9 rows: five row pairs, a second workgroup down the frame, and a last pair of one row.  The payload 1
    byte off: the last lane of a trip hands its last dword to the first lane of the next."""
    assert yg.SPAN == 1024
    frames = yc.frames_of(W, 9, 1, 5)
    yc.assert_telling(frames)
    assert_planes(YUV, frames, pad=1, shift=1, aligned=True)
    assert_planes(YUV, frames, bgr=True, poisons=(0xFF,))


@pytest.mark.parametrize('shift', range(16))
def test_every_pair_of_alignment_classes(YUV, shift):
    """37 x 17 frames, source rows at a stride of 117 and Y rows of 37 bytes, so that a frame's rows walk through all sixteen classes modulo 16
    on both sides; the payload moved `shift` bytes off its allocation: the sixteen calls reach all 256 pairs of (source class, Y row class),
    and the chroma planes, which begin 629 and 800 bytes into the payload, every class of their own."""
    W, H = 37, 17
    pairs = {((117 * y) % 16, (s + 37 * y) % 16) for s in range(16) for y in range(H)}
    assert len(pairs) == 256 and yc.frame_bytes(W, H) == 629 + 2 * 171 and len({(s + 629 + 19 * cy) % 16 for s in range(16) for cy in range(9)}) == 16
    frames = yc.frames_of(W, H, 2, 40)
    for bgr in (False, True):
        assert_planes(YUV, frames, bgr=bgr, pad=6, shift=shift, aligned=True, poisons=(0xFF,) if bgr else yg.POISONS)


def test_the_extremes(YUV):
    """All-255 and all-0 frames, and flat frames of the six primaries and secondaries, against the pinned values; 37 x 9: cells of 4, 2 and 1 pixels."""
    W, H = 37, 9
    for bgr in (False, True):
        for colour in [(255, 255, 255), (0, 0, 0)] + yc.PRIMARIES:
            frames = yc.flat(colour[::-1] if bgr else colour, W, H, 2)
            rc, got = run(YUV, frames, bgr=bgr, pad=2)
            assert rc == 0 and np.array_equal(got, yc.twin_payload(frames, bgr))
            for payload in got:
                for plane, want in zip(YUV.planes(payload, W, H), yc.PINNED.get(colour, (None, None, None))):
                    assert want is None or (plane == want).all(), (colour, bgr)
                assert all(len(np.unique(plane)) == 1 for plane in YUV.planes(payload, W, H))          # (flat in, flat out, whatever n is)
    assert {c for c in yc.PINNED} >= {(0, 0, 255), (255, 0, 0), (255, 255, 0)}


@pytest.mark.parametrize('frame', [(65535, 2), (1, 65535)], ids=lambda v: '%dx%d' % v)
def test_the_widest_and_the_tallest_frame(YUV, frame):
    """65535 x 2: one wave's 64 trips along a row pair; 1 x 65535: 32768 row pairs of one column, the last of one pixel."""
    W, H = frame
    assert_planes(YUV, yc.frames_of(W, H, 1, 3), poisons=(0xFF,), shift=3, src_shift=1)


def test_the_cut_into_launches(YUV):
    """A launch carries FRAMES_PER_LAUNCH = 12 frames: 13 frames are 12 + 1, and every payload is another."""
    W, H = 21, 6
    n = YUV.FRAMES_PER_LAUNCH + 1
    frames = yc.frames_of(W, H, n, 50)
    want = yc.twin_payload(frames)
    assert n == 13 and len({want[i].tobytes() for i in range(n)}) == n       # every payload is another: one taken for another shows
    assert_planes(YUV, frames, want)


REFUSALS = {'null frames': (lambda a: a.update(frames_u8=None), 'null frames_u8'),
            'null outputs': (lambda a: a.update(out_u8=None), 'null out_u8'),
            'n = 0': (lambda a: a.update(n_frames=0), 'n_frames < 1'),
            'W = 65536': (lambda a: a.update(W=65536, stride_bytes=3 * 65536), 'W or H outside 1..65535'),
            'H = 0': (lambda a: a.update(H=0), 'W or H outside 1..65535'),
            'stride < 3 W': (lambda a: a.update(stride_bytes=3 * a['W'] - 1), 'stride_bytes < 3 W'),
            'flags 2': (lambda a: a.update(flags=2), 'unknown bits in flags'),
            'flags 3': (lambda a: a.update(flags=3), 'unknown bits in flags'),
            'null frame 1': (lambda a: a['frames_u8'].__setitem__(1, None), 'null element of frames_u8'),
            'null output 1': (lambda a: a['out_u8'].__setitem__(1, None), 'null element of out_u8'),
            'output is a source': (lambda a: a['out_u8'].__setitem__(1, a['frames_u8'][1]), 'an element of out_u8 overlaps a source frame'),
            'output is the other outputs source': (lambda a: a['out_u8'].__setitem__(0, a['frames_u8'][1]), 'an element of out_u8 overlaps a source frame'),
            # (the frames lie a gap apart: the payload ends on the first byte of the next source and touches no other)
            'one byte of the next source': (lambda a: a['out_u8'].__setitem__(0, a['frames_u8'][1] - yc.frame_bytes(a['W'], a['H']) + 1), 'an element of out_u8 overlaps a source frame'),
            'one byte of the other output': (lambda a: a['out_u8'].__setitem__(0, a['out_u8'][1] - yc.frame_bytes(a['W'], a['H']) + 1), 'an element of out_u8 overlaps another output'),
            'the same output twice': (lambda a: a['out_u8'].__setitem__(0, a['out_u8'][1]), 'an element of out_u8 overlaps another output')}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals_leave_the_output_untouched(YUV, what):
    from ken_burns_effect_amd import _native
    W, H = yc.FRAMES[0]
    change, text = REFUSALS[what]
    rc, got = run(YUV, yc.frames_of(W, H), gap=3 * W * H + 64, change=change, poison=0xFF)
    assert rc == -1 and _native.load().kbe_last_error().decode() == 'kbe_yuv420_u8: ' + text
    assert (got == 0xFF).all()


def test_on_a_side_stream_behind_a_delay(YUV):
    """The entry called raw with the handle of a non-blocking side stream behind stream_gpu's delay: it returns while the delay runs, and the
    result is the twin, bit for bit; the sources hold a decoy until the delay has run out."""
    from ken_burns_effect_amd import _native
    n, H, W = 3, 37, 50
    right = torch.from_numpy(yc.frames_of(W, H, n, 21).copy()).cuda()
    decoy = torch.from_numpy(yc.frames_of(W, H, n, 60).copy()).cuda()
    size = YUV.frame_bytes(W, H)
    frames, out = decoy.clone(), torch.zeros(n, size, dtype=torch.uint8, device='cuda')

    def pointers(t):
        return (ctypes.c_void_p * t.shape[0])(*[t[i].data_ptr() for i in range(t.shape[0])])

    def call():
        YUV._call('kbe_yuv420_u8', pointers(frames), n, W, H, 3 * W, pointers(out), 0, _native._stream())
        return out
    what = 'yuv420_u8'
    got, want = stream_gpu.hold(what, 'bits', [frames], [right], [decoy], call, written=lambda: [out])
    assert what in stream_gpu.ENQUEUED                                      # (the entry had returned while the delay still ran)
    assert np.array_equal(got[0], yc.twin_payload(right.cpu().numpy())) and np.array_equal(got[0], want[0])


# -- the host side --------------------------------------------------------------------------------
def test_convert_and_planes_on_a_tensor(YUV):
    """13 frames of 37 x 25 -- payloads of 1419 bytes, odd, back to back in one tensor: each ends on the byte before the next begins."""
    from ken_burns_effect_amd import _native
    W, H, n = 37, 25, 13
    frames = yc.frames_of(W, H, n, 70)
    on_gpu = torch.from_numpy(frames.copy()).cuda()
    for bgr in (False, True):
        got = YUV.convert(on_gpu, bgr=bgr)
        assert got.shape == (n, YUV.frame_bytes(W, H)) == (n, 1419) and got.dtype == torch.uint8 and got.device == on_gpu.device and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), yc.twin_payload(frames, bgr))
    assert np.array_equal(YUV.convert(on_gpu).cpu().numpy(), yc.twin_payload(frames))          # bgr=False is the default
    Y, Cb, Cr = YUV.planes(got[4], W, H)
    assert Y.is_cuda and Y.shape == (H, W) and Cb.shape == Cr.shape == (13, 19) and Y.data_ptr() == got[4].data_ptr() and Cr.data_ptr() == got[4].data_ptr() + W * H + 13 * 19
    for plane, want in zip((Y, Cb, Cr), yc.twin_planes(frames[4], True)):
        assert np.array_equal(plane.cpu().numpy(), want)
    for bad in (on_gpu.cpu(), on_gpu.int(), on_gpu[:, :, ::2], on_gpu[0], on_gpu[:0], on_gpu[..., :2]):
        with pytest.raises(_native.KbeError, match=r'yuv\.convert'):
            YUV.convert(bad)


@pytest.mark.parametrize('frame', [(64, 48), (37, 25)], ids=lambda v: '%dx%d' % v)
def test_write_y4m(YUV, tmp_path, frame):
    """3 frames: the file parsed back gives the header, 5 FRAMEs forth and back -- the way back the same payloads again -- or 3 without it."""
    W, H = frame
    frames = yc.frames_of(W, H, 3, 80)
    on_gpu = torch.from_numpy(frames.copy()).cuda()
    for bgr in (False, True):
        want = yc.twin_payload(frames, bgr)
        path = str(tmp_path / ('%d.y4m' % bgr))
        assert YUV.write_y4m(path, on_gpu, bgr=bgr) == 5
        header, payloads = yc.read_y4m(path)
        assert header == b'YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n' % (W, H) == YUV.y4m_header(W, H, 25)
        assert len(payloads) == 5 and all(np.array_equal(payloads[i], want[k]) for i, k in enumerate((0, 1, 2, 1, 0)))
        assert YUV.write_y4m(path, on_gpu, fps=12.5, bgr=bgr, back=False) == 3
        header, payloads = yc.read_y4m(path)
        assert header == YUV.y4m_header(W, H, 12.5) and len(payloads) == 3 and all(np.array_equal(payloads[i], want[i]) for i in range(3))
    assert YUV.write_y4m(path, on_gpu[:1]) == 1 and len(yc.read_y4m(path)[1]) == 1                  # (one frame: there is no way back)


def _files(directory):
    return sorted(str(p.relative_to(directory)) for p in directory.rglob('*') if p.is_file())


def test_the_pipeline_with_the_switch_writes_the_y4m_beside_what_it_writes_without(YUV, tmp_path, monkeypatch):
    """One Pipeline(y4m=True, gif=True, output_frames=True, allow_random_weights=True, steps=3) call on a 64 x 48 image beside the same call
    without the switch: the same files plus 3d_kbe.y4m, equal frames returned, equal PNG files, and the y4m's payloads are the twin of the
    returned frames in BGR order, forth and back."""
    from ken_burns_effect_amd import kbe, synthetic
    from ken_burns_effect_amd.pipeline import Pipeline
    for name in ('KBE_Y4M', 'KBE_WIDTH', 'KBE_GIF', 'KBE_GIF_WIDTH', 'KBE_GIF_FPS', 'KBE_GIF_DITHER', 'KBE_PNG', 'KBE_JPEG', 'KBE_APERTURE', 'KBE_FOCUS', 'KBE_FOCUS_TO', 'KBE_SHUTTER',
                 'KBE_SHUTTER_SAMPLES'):
        monkeypatch.delenv(name, raising=False)
    image, _ = synthetic.make_rgbd(48, 64, 12)
    zoom = kbe.windows_for(64, 48, dict.fromkeys(('startU', 'startV', 'startW', 'startH', 'endU', 'endV', 'endW', 'endH')), False)
    written = {}
    for name, switch in (('plain', {}), ('y4m', dict(y4m=True))):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            pipe = Pipeline(model_paths=None, allow_random_weights=True, output_frames=True, device='cuda:0', steps=3, gif=True, **switch)
            frames = pipe(image, zoom, str(tmp_path / name))
        assert len(frames) == 3 and all(f.shape == (48, 64, 3) and f.dtype == np.uint8 for f in frames)
        written[name] = np.stack(frames)
    others = ['3d_kbe.gif', '3d_kbe.mp4', 'frames/0.png', 'frames/1.png', 'frames/2.png']
    assert _files(tmp_path / 'plain') == others and _files(tmp_path / 'y4m') == sorted(others + ['3d_kbe.y4m'])
    assert np.array_equal(written['plain'], written['y4m'])
    for name in others[2:] + ['3d_kbe.gif']:
        assert (tmp_path / 'plain' / name).read_bytes() == (tmp_path / 'y4m' / name).read_bytes(), name
    header, payloads = yc.read_y4m(str(tmp_path / 'y4m' / '3d_kbe.y4m'))
    want = yc.twin_payload(written['y4m'], bgr=True)
    assert header == YUV.y4m_header(64, 48, 25) and len(payloads) == 5
    assert all(np.array_equal(payloads[i], want[k]) for i, k in enumerate((0, 1, 2, 1, 0)))
    assert not np.array_equal(want, yc.twin_payload(written['y4m'], bgr=False)) and len({p.tobytes() for p in payloads}) == 3
